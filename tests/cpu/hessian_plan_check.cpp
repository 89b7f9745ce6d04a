// hessian_plan_check.cpp — the host-side plan of the exact energy Hessian (openvqe_amd/csrc/sv_hessian_host.hpp) compiled alone with g++
// (ASan + UBSan in tests/test_hessian_cases.py): random real rotation programs — constant angles, offsets, tied and unused parameters —
// are restated on their compact support by metric::build_compact, a random Pauli sum (identity, Z-only, even-Y and odd-Y strings) is
// restricted to THAT support, and
//   * the entries are compared with a dense restriction of Re H on the support: every pair once (ci < cj), the diagonal without the
//     identity terms, the identity terms and the caller's constant in Restricted::constant;
//   * the kernel's loop is replayed on the host exactly as k_sparse_hessian indexes its tables (every access bounds-checked) and E, the
//     gradient and the Hessian are compared with a dense complex nested-forward-mode simulation of exp(-i phi P).
//   usage: hessian_plan_check [seed]
//          hessian_plan_check boundary     cube programs at m = 4096 on both sides of the staged / unstaged / streaming decisions of the
//                                          kernel's LDS layout (sp_hessian_lds), and the refusal beyond the support cap
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>

#include "../../openvqe_amd/csrc/sv_hessian_host.hpp"

using namespace ovqe;
using cd = std::complex<double>;

static int fails = 0;
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
struct Ham {
    std::vector<uint64_t> x, z;
    std::vector<double> c;
    double constant;
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
static void axpy(std::vector<cd> &y, cd f, const std::vector<cd> &x) {
    for (size_t i = 0; i < y.size(); ++i) y[i] += f * x[i];
}
static std::vector<cd> apply_h(const Ham &H, const std::vector<cd> &a) {
    std::vector<cd> out(a.size(), 0.0);
    for (size_t t = 0; t < H.x.size(); ++t) axpy(out, H.c[t], pauli(a, H.x[t], H.z[t]));
    return out;
}
static cd dot(const std::vector<cd> &a, const std::vector<cd> &b) {
    cd s = 0.0;
    for (size_t i = 0; i < a.size(); ++i) s += std::conj(a[i]) * b[i];
    return s;
}

// the grouped terms as the library builds them (build_groups): sorted by x, i^ny folded into cr + i ci
static void group_terms(const Ham &H, std::vector<HGroup> &groups, std::vector<HTerm> &terms) {
    std::vector<size_t> order(H.x.size());
    for (size_t t = 0; t < order.size(); ++t) order[t] = t;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return H.x[a] < H.x[b]; });
    for (size_t oi = 0; oi < order.size(); ++oi) {
        const size_t t = order[oi];
        const int ny = __builtin_popcountll(H.x[t] & H.z[t]) & 3;
        const double c = H.c[t];
        HTerm ht{H.z[t], ny == 0 ? c : ny == 2 ? -c : 0.0, ny == 1 ? c : ny == 3 ? -c : 0.0};
        if (groups.empty() || H.x[order[oi - 1]] != H.x[t]) groups.push_back(HGroup{H.x[t], 0, (int32_t)terms.size(), (int32_t)terms.size(), 0.0});
        terms.push_back(ht);
        groups.back().t1 = (int32_t)terms.size();
    }
}

static Ham random_ham(std::mt19937_64 &rng, int n, int T) {
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    const uint64_t N = 1ull << n;
    Ham H;
    H.constant = U(rng);
    auto push = [&](uint64_t x, uint64_t z) {
        H.x.push_back(x);
        H.z.push_back(z);
        H.c.push_back(U(rng));
    };
    push(0, 0);                         // identity
    push(0, 1 + rng() % (N - 1));       // Z only
    push(0, 0);                         // a second identity term: both go to the constant
    while ((int)H.x.size() < T) push(rng() & (N - 1), rng() & (N - 1));   // even and odd numbers of Y
    return H;
}

// the kernel's dynamic LDS is sp_hessian_lds itself (sv_sparse_layout.hpp: the header the kernel and its launcher read); the layout
// does not depend on the entry count or the constant
static SpHessLds lds_layout(const metric::Compact &C, int K, bool stage) { return sp_hessian_lds(sp_hessian_args(C, K, 0, 0.0), stage); }
constexpr size_t LDS_BUDGET = 150 * 1024, LDS_MAX = 160 * 1024;   // LDS_WG_BUDGET / LDS_WG_MAX of ovqe_sv.hip

static bool compact_of(uint64_t hf, const std::vector<Rot> &prog, int K, metric::Compact *C) {
    std::vector<metric::InOp> ops;
    std::vector<metric::InRot> rots;
    for (size_t r = 0; r < prog.size();) {   // same-x runs, unfused (metric_plan_check.cpp covers the fused tables)
        size_t e = r + 1;
        while (e < prog.size() && prog[e].x == prog[r].x) ++e;
        ops.push_back(metric::InOp{prog[r].x, 0, metric::KIND_ROT, (int)rots.size(), (int)(e - r)});
        for (size_t q = r; q < e; ++q)
            rots.push_back(metric::InRot{prog[q].z, prog[q].coeff, prog[q].phi0, prog[q].pidx, (int)(__builtin_popcountll(prog[q].x & prog[q].z) & 3)});
        r = e;
    }
    return metric::build_compact(hf, ops, rots, K, C);
}

// the entries against the dense restriction
static void check_entries(int n, const metric::Compact &C, const Ham &H, const hessian::Restricted &R) {
    const uint64_t N = 1ull << n;
    const int m = C.m;
    CHECK((int)C.support.size() == m && C.support[(size_t)C.hf] < N, "support list");
    double want_const = H.constant;
    std::vector<double> dense((size_t)m * m, 0.0);
    for (size_t t = 0; t < H.x.size(); ++t) {
        if (H.x[t] == 0 && H.z[t] == 0) {
            want_const += H.c[t];
            continue;
        }
        for (int l = 0; l < m; ++l) {
            std::vector<cd> e(N, 0.0);
            e[C.support[(size_t)l]] = 1.0;
            const std::vector<cd> p = pauli(e, H.x[t], H.z[t]);
            for (int k = 0; k < m; ++k) dense[(size_t)k * m + l] += (H.c[t] * p[C.support[(size_t)k]]).real();
        }
    }
    CHECK(std::fabs(R.constant - want_const) < 1e-14, "constant %.17g, want %.17g", R.constant, want_const);
    std::vector<double> got((size_t)m * m, 0.0);
    std::set<uint32_t> seen;
    for (const hessian::Entry &en : R.entries) {
        const uint32_t ci = en.ij & 0xfffu, cj = (en.ij >> 12) & 0xfffu;
        CHECK(ci < (uint32_t)m && cj < (uint32_t)m && ci <= cj && (en.ij >> 24) == 0 && en.pad == 0, "entry out of range");
        CHECK(seen.insert(en.ij).second, "pair (%u, %u) listed twice", ci, cj);
        if (ci >= (uint32_t)m || cj >= (uint32_t)m) continue;
        if (ci == cj) got[(size_t)ci * m + ci] = en.c;
        else got[(size_t)ci * m + cj] = got[(size_t)cj * m + ci] = 0.5 * en.c;
    }
    double worst = 0.0;
    for (size_t i = 0; i < dense.size(); ++i) worst = std::max(worst, std::fabs(dense[i] - got[i]));
    CHECK(worst < 1e-13, "restricted Hamiltonian differs from the dense restriction by %.3e (m = %d)", worst, m);
}

// k_sparse_hessian's loop on the host -> raw rows M, gradient, energy
static void replay(const metric::Compact &C, const hessian::Restricted &R, const std::vector<double> &theta, int K, std::vector<double> &M,
                   std::vector<double> &grad, double *energy) {
    const int nops = (int)C.ops.size(), ntab = (int)C.tab.size(), m = C.m;
    const SpHessLds L = lds_layout(C, K, true);
    CHECK(L.cs % 16 == 0 && L.ops % 16 == 0 && L.gk + (size_t)K * 8 <= L.ops && L.pairs + C.pairs.size() * 4 == L.bytes, "LDS regions");
    M.assign((size_t)K * K, 0.0);
    grad.assign((size_t)K, 0.0);
    for (int b = 0; b < K; ++b) {
        std::vector<double> psi((size_t)m, 0.0), t((size_t)m, 0.0), lam((size_t)m, 0.0), mu((size_t)m, 0.0);
        std::vector<double> c((size_t)ntab), s((size_t)ntab), dk((size_t)ntab), w((size_t)ntab, 0.0), wd((size_t)ntab, 0.0), gk((size_t)K, 0.0);
        psi.at((size_t)C.hf) = 1.0;
        for (int e = 0; e < ntab; ++e) {
            const metric::TabEntry &te = C.tab[(size_t)e];
            const double phi = te.phi0 + (te.pidx >= 0 ? te.coeff * theta.at((size_t)te.pidx) : 0.0);
            c[(size_t)e] = std::cos(phi);
            s[(size_t)e] = std::sin(phi);
            dk[(size_t)e] = te.pidx == b ? te.coeff : 0.0;
        }
        const int o1 = std::min(C.first_op.at((size_t)b), nops);
        for (int o = 0; o < nops; ++o) {
            const metric::Op &op = C.ops[(size_t)o];
            for (int pe = 0; pe < op.npairs; ++pe) {
                const uint32_t pw = C.pairs.at((size_t)(op.first + pe));
                const uint32_t ci = pw & 0xfffu, cj = (pw >> 12) & 0xfffu;
                const size_t e = (size_t)op.tab0 + (pw >> 25);
                const bool neg = (pw >> 24) & 1u;
                const double sn = neg ? -s.at(e) : s.at(e), d = neg ? -dk.at(e) : dk.at(e);
                const double u = psi.at(ci), v = psi.at(cj), tu = t.at(ci), tv = t.at(cj);
                const double u1 = c[e] * u + sn * v, v1 = c[e] * v - sn * u;
                psi[ci] = u1;
                psi[cj] = v1;
                if (o >= o1) {
                    t[ci] = c[e] * tu + sn * tv + d * v1;
                    t[cj] = c[e] * tv - sn * tu - d * u1;
                } else CHECK(d == 0.0, "first_op skips an op that holds an entry of parameter %d", b);
            }
        }
        double acc = 0.0;
        for (const hessian::Entry &en : R.entries) {
            const uint32_t ci = en.ij & 0xfffu, cj = (en.ij >> 12) & 0xfffu;
            acc += en.c * psi.at(ci) * psi.at(cj);
            if (ci == cj) {
                lam[ci] += en.c * psi[ci];
                mu[ci] += en.c * t[ci];
            } else {
                lam[ci] += 0.5 * en.c * psi[cj];
                lam[cj] += 0.5 * en.c * psi[ci];
                mu[ci] += 0.5 * en.c * t[cj];
                mu[cj] += 0.5 * en.c * t[ci];
            }
        }
        if (b == 0) *energy = acc + R.constant;
        for (int o = nops - 1; o >= 0; --o) {
            const metric::Op &op = C.ops[(size_t)o];
            for (int pe = 0; pe < op.npairs; ++pe) {
                const uint32_t pw = C.pairs.at((size_t)(op.first + pe));
                const uint32_t ci = pw & 0xfffu, cj = (pw >> 12) & 0xfffu;
                const size_t e = (size_t)op.tab0 + (pw >> 25);
                const bool neg = (pw >> 24) & 1u;
                const double sn = neg ? -s.at(e) : s.at(e), d = neg ? -dk.at(e) : dk.at(e);
                const double u1 = psi.at(ci), v1 = psi.at(cj), lu = lam.at(ci), lv = lam.at(cj);
                const double tu = o >= o1 ? t.at(ci) : 0.0, tv = o >= o1 ? t.at(cj) : 0.0, mu1 = mu.at(ci), mv1 = mu.at(cj);
                const double gd = mu1 * v1 - mv1 * u1 + lu * tv - lv * tu, g = lu * v1 - lv * u1;
                wd.at(e) += neg ? -gd : gd;
                w.at(e) += neg ? -g : g;
                const double u0 = c[e] * u1 - sn * v1, v0 = c[e] * v1 + sn * u1, lu0 = c[e] * lu - sn * lv, lv0 = c[e] * lv + sn * lu;
                psi[ci] = u0;
                psi[cj] = v0;
                lam[ci] = lu0;
                lam[cj] = lv0;
                if (o >= o1) {
                    t[ci] = c[e] * tu - sn * tv - d * v0;
                    t[cj] = c[e] * tv + sn * tu + d * u0;
                }
                mu[ci] = c[e] * mu1 - sn * mv1 - (o >= o1 ? d * lv0 : 0.0);
                mu[cj] = c[e] * mv1 + sn * mu1 + (o >= o1 ? d * lu0 : 0.0);
            }
        }
        for (int e = 0; e < ntab; ++e) {
            const metric::TabEntry &te = C.tab[(size_t)e];
            if (te.pidx < 0) continue;
            gk.at((size_t)te.pidx) += 2.0 * te.coeff * wd[(size_t)e];
            if (b == 0) grad.at((size_t)te.pidx) += 2.0 * te.coeff * w[(size_t)e];
        }
        for (int k = 0; k < K; ++k) M[(size_t)b * K + k] = gk[(size_t)k];
    }
}

// dense nested forward mode: psi, T_k, T_bk through the program; H_bk = 2 Re <T_b|H|T_k> + 2 Re <psi|H|T_bk>
static void dense_hessian(int n, uint64_t hf, const std::vector<Rot> &prog, const std::vector<double> &theta, int K, const Ham &H,
                          std::vector<double> &hess, std::vector<double> &grad, double *energy) {
    const uint64_t N = 1ull << n;
    std::vector<cd> psi(N, 0.0);
    psi[hf] = 1.0;
    std::vector<std::vector<cd>> T((size_t)K, std::vector<cd>(N, 0.0)), S((size_t)K * K, std::vector<cd>(N, 0.0));
    const cd mi(0, -1);
    for (const Rot &q : prog) {
        const double phi = q.phi0 + (q.pidx >= 0 ? q.coeff * theta[(size_t)q.pidx] : 0.0);
        rotate(psi, q.x, q.z, phi);
        for (auto &t : T) rotate(t, q.x, q.z, phi);
        for (auto &s : S) rotate(s, q.x, q.z, phi);
        if (q.pidx < 0) continue;
        const size_t p = (size_t)q.pidx;
        const std::vector<cd> Ppsi = pauli(psi, q.x, q.z);
        for (size_t k = 0; k < (size_t)K; ++k) {
            const std::vector<cd> PT = pauli(T[k], q.x, q.z);
            axpy(S[p * K + k], mi * q.coeff, PT);
            axpy(S[k * K + p], mi * q.coeff, PT);
        }
        axpy(S[p * K + p], -q.coeff * q.coeff, psi);   // c^2 (-i P)^2 psi
        axpy(T[p], mi * q.coeff, Ppsi);
    }
    const std::vector<cd> lam = apply_h(H, psi);
    *energy = dot(psi, lam).real() + H.constant;
    hess.assign((size_t)K * K, 0.0);
    grad.assign((size_t)K, 0.0);
    std::vector<std::vector<cd>> HT;
    for (auto &t : T) HT.push_back(apply_h(H, t));
    for (int b = 0; b < K; ++b) {
        grad[(size_t)b] = 2.0 * dot(lam, T[(size_t)b]).real();
        for (int k = 0; k < K; ++k) hess[(size_t)b * K + k] = 2.0 * dot(T[(size_t)b], HT[(size_t)k]).real() + 2.0 * dot(lam, S[(size_t)b * K + k]).real();
    }
}

static void one_program(std::mt19937_64 &rng, int n, int R, int K) {
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    const uint64_t N = 1ull << n, hf = rng() & (N - 1);
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
        // the first rotations are constants, so that some direction's first op is not op 0; the last parameter stays unused
        q.pidx = (r < 2 || rng() % 7 == 0) ? -1 : (int)(rng() % (uint64_t)std::max(K - 1, 1));
        q.coeff = U(rng);
        q.phi0 = (rng() % 3 == 0 || q.pidx < 0) ? U(rng) : 0.0;
        prog.push_back(q);
    }
    std::vector<double> theta((size_t)K);
    for (double &t : theta) t = U(rng);
    metric::Compact C;
    CHECK(compact_of(hf, prog, K, &C), "build_compact declined a real program (n = %d)", n);
    const Ham H = random_ham(rng, n, 14);
    std::vector<HGroup> groups;
    std::vector<HTerm> terms;
    group_terms(H, groups, terms);
    hessian::Restricted Rs;
    CHECK(hessian::restrict_hamiltonian(C.support, groups, terms, H.constant, (size_t)1 << 20, &Rs), "restriction declined");
    check_entries(n, C, H, Rs);
    hessian::Restricted tiny;
    if (Rs.entries.size() > 1) CHECK(!hessian::restrict_hamiltonian(C.support, groups, terms, H.constant, Rs.entries.size() - 1, &tiny), "entry cap ignored");
    std::vector<double> M, g, hd, gd;
    double e = 0.0, ed = 0.0;
    replay(C, Rs, theta, K, M, g, &e);
    dense_hessian(n, hf, prog, theta, K, H, hd, gd, &ed);
    double h1 = std::fabs(H.constant), cmax = 0.0;
    for (double c : H.c) h1 += std::fabs(c);
    std::vector<double> csum((size_t)K, 0.0);
    for (const Rot &q : prog)
        if (q.pidx >= 0) cmax = std::max(cmax, csum[(size_t)q.pidx] += std::fabs(q.coeff));
    const double tol = 1e-12 * h1 * std::max(1.0, cmax * cmax);
    CHECK(std::fabs(e - ed) < 1e-13 * h1, "energy %.17g, dense %.17g", e, ed);
    double worst = 0.0, asym = 0.0, wg = 0.0;
    bool later = false;
    for (int b = 0; b < K; ++b) {
        wg = std::max(wg, std::fabs(g[(size_t)b] - gd[(size_t)b]));
        later = later || (C.first_op[(size_t)b] > 0 && C.first_op[(size_t)b] < (int)C.ops.size());
        for (int k = 0; k < K; ++k) {
            worst = std::max(worst, std::fabs(M[(size_t)b * K + k] - hd[(size_t)b * K + k]));
            asym = std::max(asym, std::fabs(M[(size_t)b * K + k] - M[(size_t)k * K + b]));
        }
    }
    CHECK(later, "no direction starts behind op 0");
    CHECK(wg < tol, "gradient differs from the dense simulation by %.3e", wg);
    CHECK(worst < tol && asym < tol, "Hessian differs from the dense simulation by %.3e, asymmetry %.3e (n = %d, K = %d, tol %.3e)", worst, asym, n, K, tol);
    if (K >= 2)   // the unused last parameter: an exact zero row and column
        for (int k = 0; k < K; ++k) CHECK(M[(size_t)(K - 1) * K + k] == 0.0 && M[(size_t)k * K + (K - 1)] == 0.0, "unused parameter");
}

// cube program of metric_plan_check.cpp: a single Y on bit r for r < n, then odd-Y strings of weight 2..5, every rotation with an offset
static std::vector<Rot> cube_program(std::mt19937_64 &rng, int n, int R, int K) {
    std::uniform_real_distribution<double> U(0.2, 1.0);
    std::vector<Rot> prog;
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
                    const int letter = (int)(rng() % 3);
                    if (letter != 2) q.x |= bit;
                    if (letter != 0) q.z |= bit;
                }
                if (__builtin_popcountll(q.x & q.z) & 1) break;
            }
        }
        q.pidx = r <= K ? r - 1 : (int)(rng() % (uint64_t)(K + 1)) - 1;
        q.coeff = ((rng() & 1) ? 0.3 : -0.3) * (0.1 + U(rng));
        q.phi0 = ((rng() & 1) ? 1.0 : -1.0) * U(rng);
        prog.push_back(q);
    }
    return prog;
}

static int form_of(const metric::Compact &C, int K) {
    return lds_layout(C, K, true).bytes <= LDS_BUDGET ? 1 : lds_layout(C, K, false).bytes <= LDS_BUDGET ? 2 : 0;
}

static void boundary() {
    std::mt19937_64 rng(12);
    const int n = 12, K = 6;
    // the four programs around the two decisions: found from the layout and the program's sizes, then built and confirmed
    std::vector<int> Rs;
    {
        // sizes of the cube program: one op and one table entry per rotation, rotation r < n pairs 2^r states with 2^r new ones, every
        // later one the whole register
        auto form = [&](int r) {
            metric::Compact C;
            C.m = 1 << n;
            C.tab.resize((size_t)r);
            C.ops.resize((size_t)r);
            C.pairs.resize((size_t)((1 << n) - 1 + (r - n) * (1 << (n - 1))));
            return form_of(C, K);
        };
        int R = n;
        CHECK(form(R) == 1, "the shortest cube program is not staged");
        while (form(R + 1) == 1) ++R;
        Rs.push_back(R);
        Rs.push_back(R + 1);
        R += 1;
        while (form(R + 1) == 2) ++R;
        Rs.push_back(R);
        Rs.push_back(R + 1);
    }
    const int want_form[4] = {1, 2, 2, 0};
    for (int k = 0; k < 4; ++k) {
        const int R = Rs[(size_t)k];
        metric::Compact C;
        const bool ok = compact_of(rng() & 4095, cube_program(rng, n, R, K), K, &C);
        CHECK(ok, "build_compact declined the cube program R = %d", R);
        if (!ok) continue;
        uint32_t max_c = 0;
        for (const uint32_t pw : C.pairs) max_c = std::max(max_c, std::max(pw & 0xfffu, (pw >> 12) & 0xfffu));
        CHECK(C.m == metric::MAX_SUPPORT && max_c == 4095u && (int)C.support.size() == C.m, "m = %d, max index %u", C.m, max_c);
        CHECK((int)C.tab.size() == R && (int)C.ops.size() == R, "one op and one table entry per rotation");
        const SpHessLds Ls = lds_layout(C, K, true), Lu = lds_layout(C, K, false);
        const int form = form_of(C, K);
        CHECK(form == want_form[k], "R = %d: form %d, want %d", R, form, want_form[k]);
        const SpHessLds &L = form == 1 ? Ls : Lu;
        CHECK(((size_t)max_c + 1) * 8 <= L.t && L.mu + L.t == L.cs && L.cs % 16 == 0 && L.ops % 16 == 0, "vector regions");
        CHECK(L.cs + C.tab.size() * 16 == L.dk && L.wd + C.tab.size() * 8 == L.gk && L.gk + (size_t)K * 8 <= L.ops, "table regions");
        if (form == 1) CHECK(L.ops + C.ops.size() * 16 == L.pairs && L.pairs + C.pairs.size() * 4 == L.bytes, "staged regions");
        if (form) CHECK(L.bytes <= LDS_BUDGET && L.bytes <= LDS_MAX, "the launch exceeds the budget");
        // the restricted Hamiltonian at the cap: compact index 4095 in the 12-bit fields of an entry
        Ham H = random_ham(rng, n, 12);
        std::vector<HGroup> groups;
        std::vector<HTerm> terms;
        group_terms(H, groups, terms);
        hessian::Restricted Rr;
        CHECK(hessian::restrict_hamiltonian(C.support, groups, terms, H.constant, (size_t)1 << 24, &Rr), "restriction declined at the cap");
        uint32_t max_e = 0;
        for (const hessian::Entry &en : Rr.entries) max_e = std::max(max_e, (en.ij >> 12) & 0xfffu);
        CHECK(max_e == 4095u && (Rr.entries.empty() || (Rr.entries.back().ij >> 24) == 0), "entries at the cap: max cj %u", max_e);
        std::printf("cube n=%d R=%d ok=1 m=%d ntab=%zu nops=%zu npairs=%zu staged=%zu unstaged=%zu form=%d entries=%zu\n", n, R, C.m, C.tab.size(),
                    C.ops.size(), C.pairs.size(), Ls.bytes, Lu.bytes, form, Rr.entries.size());
    }
    // the streaming workspace: both stores, at most 256 slabs of at least four rows, one weight record per parameterised rotation + 1
    {
        const hessian::Streaming a = hessian::streaming_layout(1 << 14, 3, 4), b = hessian::streaming_layout(32, 5, 9), c = hessian::streaming_layout(4096, 6, 500);
        CHECK(a.slab_rows == 64 && a.nslabs == 256 && a.bytes == (size_t)2 * 16384 * 64 * 16 + 256 * 64 * 8 + 4 * 64 * 8, "14-qubit streaming workspace");
        CHECK(b.slab_rows == 4 && b.nslabs == 8 && b.bytes == (size_t)2 * 32 * 64 * 16 + 8 * 64 * 8 + 9 * 64 * 8, "5-qubit streaming workspace");
        CHECK(c.slab_rows * c.nslabs >= 4096 && c.nslabs <= 256 && c.part_bytes == (size_t)c.nslabs * 64 * 8 && c.w_bytes == (size_t)500 * 64 * 8, "slabs cover the rows");
        CHECK(hessian::streaming_layout(1 << 12, 64, 2).store_bytes == (size_t)4096 * 128 * 16, "K + 1 columns padded to the Gram block");
    }
    // one qubit more: the 13th Y rotation reaches state 4097 and the compact program is refused
    {
        metric::Compact C;
        const bool ok = compact_of(5, cube_program(rng, 13, 13, K), K, &C);
        CHECK(!ok, "a support of 8192 states accepted");
        std::printf("cube n=13 R=13 ok=%d\n", (int)ok);
    }
}

int main(int argc, char **argv) {
    if (argc > 1 && !std::strcmp(argv[1], "boundary")) {
        boundary();
        if (fails) {
            std::printf("hessian plan: %d failures\n", fails);
            return 1;
        }
        std::printf("hessian plan boundary ok\n");
        return 0;
    }
    std::mt19937_64 rng(argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1);
    int programs = 0;
    for (int rep = 0; rep < 4; ++rep)
        for (int K : {1, 2, 3, 5}) {
            const int n = 4 + (int)(rng() % 3);
            one_program(rng, n, 10 + (int)(rng() % 8), K);
            ++programs;
        }
    if (fails) {
        std::printf("hessian plan: %d failures\n", fails);
        return 1;
    }
    std::printf("hessian plan ok (%d programs)\n", programs);
    return 0;
}
