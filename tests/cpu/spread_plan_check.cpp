// spread_plan_check.cpp — the launch planner and the eligibility rule of the energy spread (openvqe_amd/csrc/sv_spread_host.hpp) and the
// kernel's LDS layout (sp_spread_batch_lds, sv_sparse_layout.hpp) compiled alone with g++ (ASan + UBSan in tests/test_spread_cases.py).
//   usage: spread_plan_check FILE             FILE: one case per line, "m ntab nops npairs K B waves workgroups cus"
//          spread_plan_check --closure FILE   FILE: "S T", then S support states, then T terms "x z coeff" (real coefficients)
// First form: for every case the layout's regions are checked (16-byte strides, three state arrays and the tables of a wave that do not
// overlap, the shared tables behind the last wave, the gradient kernel's layout untouched) and the planner's choice is printed for the
// test to compare with its Python restatement (tests/spread_cases.py).  Second form: the terms are grouped by x mask as the library
// groups them (i^ny folded, tiny = 64 eps sum |c|) and spread::exactness is printed.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <unordered_set>
#include <vector>

#include "../../openvqe_amd/csrc/sv_spread_host.hpp"

using namespace ovqe;

static int fails = 0;
#define CHECK(cond, ...)                                     \
    do {                                                     \
        if (!(cond)) {                                       \
            std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                        \
            std::printf("\n");                               \
            if (++fails > 20) std::exit(1);                  \
        }                                                    \
    } while (0)

static void check_layout(const SparseArgs &A, int nw, bool stage) {
    const SpSpreadBatchLds L = sp_spread_batch_lds(A, nw, stage);
    const size_t v = (size_t)A.mpad * 8, keven = (size_t)((A.K + 1) & ~1) * 8;
    CHECK(L.lam == v && L.mu == 2 * v && L.cs == 3 * v && L.cs % 16 == 0, "vector regions");
    CHECK(L.w == L.cs + (size_t)A.ntab * 16 && L.gk == L.w + (size_t)A.ntab * 8, "table regions");
    CHECK(L.stride % 16 == 0 && L.stride >= L.gk + keven && L.stride < L.gk + keven + 16, "stride %zu", L.stride);
    CHECK(L.ops == (size_t)nw * L.stride && L.ops % 16 == 0 && L.pairs == L.ops + (size_t)A.nops * 16, "shared tables behind the last wave");
    CHECK(L.bytes == (stage ? L.pairs + (size_t)A.npairs * 4 : L.ops), "bytes");
    // one more state array than the gradient kernel's region, nothing else
    const SpGradBatchLds G = sp_grad_batch_lds(A, nw, stage);
    CHECK(G.lam == v && G.cs == 2 * v && L.stride == G.stride + v, "the gradient kernel's layout plus one array");
}

static void check_rows(int64_t B, int nw, int64_t grid) {
    if (B > 4096) return;
    std::vector<int> seen((size_t)B, 0);
    for (int64_t g = 0; g < grid; ++g)
        for (int v = 0; v < nw; ++v)
            for (int64_t b = g * nw + v; b < B; b += grid * nw) ++seen[(size_t)b];
    for (int64_t b = 0; b < B; ++b) CHECK(seen[(size_t)b] == 1, "row %lld visited %d times", (long long)b, seen[(size_t)b]);
}

static int plan_cases(const char *path) {
    std::FILE *f = std::fopen(path, "r");
    if (!f) return 2;
    long long v[9];
    int cases = 0;
    while (std::fscanf(f, "%lld %lld %lld %lld %lld %lld %lld %lld %lld", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7, v + 8) == 9) {
        SparseArgs A = {};
        A.m = (int)v[0];
        A.mpad = (A.m + 1) & ~1;
        A.ntab = (int)v[1];
        A.nops = (int)v[2];
        A.npairs = (int)v[3];
        A.K = (int)v[4];
        A.B = v[5];
        for (int nw : {1, 2, 4, 8})
            for (bool stage : {true, false}) check_layout(A, nw, stage);
        const gradbatch::Plan P = spread::plan(A, A.B, (int)v[6], v[7], (int)v[8]);
        CHECK(P.ok == spread::fits(A), "a plan exactly for the programs whose region fits");
        CHECK(!spread::fits(A) || gradbatch::eligible(A), "a program that fits three arrays fits two");
        if (P.ok) {
            CHECK(P.lds == sp_spread_batch_lds(A, P.nw, P.stage).bytes && P.lds <= gradbatch::LDS_BUDGET, "the launch exceeds the budget");
            CHECK(P.per_cu >= 1 && (size_t)P.per_cu * P.lds <= gradbatch::LDS_CU && P.per_cu * P.nw <= spread::waves_cu(P.stage), "residency");
            CHECK(P.workgroups >= 1 && (P.workgroups - 1) * P.nw < std::max<int64_t>(A.B, 1), "a workgroup without a row");
            CHECK(v[7] <= 0 || P.workgroups <= v[7], "the cap on the grid");
            check_rows(A.B, P.nw, P.workgroups);
        }
        std::printf("case m=%d ntab=%d nops=%d npairs=%d K=%d B=%lld waves=%lld cap=%lld cus=%lld fits=%d ok=%d nw=%d stage=%d per_cu=%d workgroups=%lld lds=%zu\n",
                    A.m, A.ntab, A.nops, A.npairs, A.K, v[5], v[6], v[7], v[8], (int)spread::fits(A), (int)P.ok, P.nw, (int)P.stage, P.per_cu,
                    (long long)P.workgroups, P.lds);
        ++cases;
    }
    std::fclose(f);
    if (fails) {
        std::printf("spread plan: %d failures\n", fails);
        return 1;
    }
    std::printf("spread plan ok (%d cases)\n", cases);
    return 0;
}

static int closure_case(const char *path) {
    std::FILE *f = std::fopen(path, "r");
    if (!f) return 2;
    long long ns = 0, nt = 0;
    if (std::fscanf(f, "%lld %lld", &ns, &nt) != 2 || ns < 0 || nt < 0) return 2;
    std::vector<uint64_t> S((size_t)ns), x((size_t)nt), z((size_t)nt);
    std::vector<double> c((size_t)nt);
    for (auto &a : S) {
        unsigned long long t = 0;
        if (std::fscanf(f, "%llu", &t) != 1) return 2;
        a = t;
    }
    for (size_t t = 0; t < (size_t)nt; ++t) {
        unsigned long long xx = 0, zz = 0;
        if (std::fscanf(f, "%llu %llu %lf", &xx, &zz, &c[t]) != 3) return 2;
        x[t] = xx;
        z[t] = zz;
    }
    std::fclose(f);
    // the library's grouping: terms sorted by x (stable), i^ny folded into the coefficient, one group per x
    std::vector<size_t> order((size_t)nt);
    std::iota(order.begin(), order.end(), (size_t)0);
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return x[a] < x[b]; });
    std::vector<HGroup> groups;
    std::vector<HTerm> terms;
    for (size_t oi = 0; oi < order.size(); ++oi) {
        const size_t t = order[oi];
        HTerm ht;
        ht.z = z[t];
        fold_iny(c[t], 0.0, __builtin_popcountll(x[t] & z[t]), ht.cr, ht.ci);
        if (groups.empty() || x[order[oi - 1]] != x[t]) {
            HGroup g = {};
            g.x = x[t];
            g.t0 = g.t1 = (int32_t)terms.size();
            groups.push_back(g);
        }
        terms.push_back(ht);
        groups.back().t1 = (int32_t)terms.size();
        groups.back().tiny += 64.0 * 2.220446049250313e-16 * (std::fabs(ht.cr) + std::fabs(ht.ci));
    }
    const std::unordered_set<uint64_t> in(S.begin(), S.end());
    const spread::Exactness E = spread::exactness(groups, terms, S, [&](uint64_t a) { return in.count(a) != 0; });
    std::printf("closure states=%lld terms=%lld groups=%zu odd_y=%d leak=%d\n", ns, nt, groups.size(), (int)E.odd_y, (int)E.leak);
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 3 && !std::strcmp(argv[1], "--closure")) return closure_case(argv[2]);
    if (argc != 2) return 2;
    return plan_cases(argv[1]);
}
