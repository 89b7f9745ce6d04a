// measure_plan_check.cpp — the host-only plan of finite-shot measurement (openvqe_amd/csrc/sv_measure_host.hpp) under ASan + UBSan with
// g++ alone (tests/test_measure_cases.py builds and runs it).
//
//   measure_plan_check CASES    CASES: a text file of term lists, per case one line "n T" and T lines "x z coeff" (masks in hex, the
//                               coefficient as a C99 hex float)
// Per case it checks the plan against the rule's consequences — every non-identity term in exactly one group, members listed once,
// every term equal to its group's basis on each of its bits, bases disjoint and inside the register, the geometry of every group's
// basis change consistent — and prints the plan ("case G", the groups of the terms, the bases) for the caller to compare with its
// own restatement of the rule.  Ends with "measure plan ok".
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "../../openvqe_amd/csrc/sv_measure_host.hpp"

using namespace ovqe;

#define REQUIRE(c)                                                        \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::printf("FAILED %s (line %d, case %d)\n", #c, __LINE__, ncase); \
            return 1;                                                     \
        }                                                                 \
    } while (0)

int main(int argc, char **argv) {
    int ncase = 0;
    if (argc < 2) return 2;
    std::FILE *f = std::fopen(argv[1], "r");
    if (!f) return 2;
    int n;
    long long T;
    while (std::fscanf(f, "%d %lld", &n, &T) == 2) {
        std::vector<uint64_t> x((size_t)T), z((size_t)T);
        std::vector<double> c((size_t)T);
        for (long long t = 0; t < T; ++t) {
            char buf[64];
            REQUIRE(std::fscanf(f, "%" SCNx64 " %" SCNx64 " %63s", &x[t], &z[t], buf) == 3);
            c[t] = std::strtod(buf, nullptr);
        }
        const measure::Plan P = measure::plan_groups(T, x.data(), z.data(), c.data());
        const int G = P.groups();
        REQUIRE((long long)P.group_of_term.size() == T && (int)P.ybasis.size() == G && (int)P.first.size() == G + 1);
        std::multiset<int32_t> seen(P.members.begin(), P.members.end());
        double constant = 0.0;
        for (long long t = 0; t < T; ++t) {
            const int g = P.group_of_term[t];
            if (!(x[t] | z[t])) {
                REQUIRE(g == -1 && seen.count((int32_t)t) == 0);
                constant += c[t];
                continue;
            }
            REQUIRE(g >= 0 && g < G && seen.count((int32_t)t) == 1);
            bool listed = false;
            for (int64_t k = P.first[g]; k < P.first[g + 1]; ++k) listed = listed || P.members[k] == t;
            REQUIRE(listed);
            const uint64_t tx = x[t] & ~z[t], ty = x[t] & z[t], tz = z[t] & ~x[t];
            REQUIRE(!(tx & ~P.xbasis[g]) && !(ty & ~P.ybasis[g]) && !(tz & (P.xbasis[g] | P.ybasis[g])));
        }
        REQUIRE(constant == P.constant);
        std::printf("case %d\n", G);
        for (long long t = 0; t < T; ++t) std::printf("%d ", P.group_of_term[t]);
        std::printf("\n");
        for (int g = 0; g < G; ++g) {
            REQUIRE(measure::basis_ok(n, P.xbasis[g], P.ybasis[g]));
            REQUIRE(P.first[g + 1] > P.first[g]);
            for (int64_t k = P.first[g] + 1; k < P.first[g + 1]; ++k)   // members in joining order: |coeff| descending
                REQUIRE(std::fabs(c[P.members[k - 1]]) >= std::fabs(c[P.members[k]]));
            const measure::Geometry Q = measure::geometry(n, P.xbasis[g], P.ybasis[g]);
            uint64_t rebuilt_x = Q.low_x, rebuilt_y = Q.low_y;
            REQUIRE(Q.high.size() == Q.high_y.size());
            for (size_t k = 0; k < Q.high.size(); ++k) {
                REQUIRE(Q.high[k] >= Q.tile_bits && Q.high[k] < n);
                (Q.high_y[k] ? rebuilt_y : rebuilt_x) |= 1ull << Q.high[k];
            }
            REQUIRE(rebuilt_x == P.xbasis[g] && rebuilt_y == P.ybasis[g]);
            REQUIRE((Q.tiles << Q.tile_bits) == (1ull << n) && Q.chunks * measure::SCAN_CHUNK >= (1ull << n));
            std::printf("%" PRIx64 " %" PRIx64 "\n", P.xbasis[g], P.ybasis[g]);
        }
        ++ncase;
    }
    std::fclose(f);
    // the basis masks that are refused, and the estimator on equal values
    REQUIRE(!measure::basis_ok(4, 3, 1) && !measure::basis_ok(4, 16, 0) && !measure::basis_ok(4, 0, 1ull << 63) && measure::basis_ok(4, 5, 10));
    REQUIRE(measure::basis_ok(64, ~0ull, 0));
    {
        const measure::Geometry Q = measure::geometry(16, 0x8801, 0x4002);
        REQUIRE(Q.tile_bits == 11 && Q.low_x == 0x1 && Q.low_y == 0x2 && Q.high.size() == 3 && Q.high[0] == 11 && Q.high_y[1] == 1 && Q.chunks == 32);
        const measure::Geometry S = measure::geometry(1, 1, 0);
        REQUIRE(S.tile_bits == 1 && S.tiles == 1 && S.high.empty() && S.chunks == 1);
    }
    double e = 0.0, s = 1.0;
    measure::estimate(0.25, 4096, {4096 * 0.3, -4096 * 1.7}, {4096 * (0.3 * 0.3), 4096 * (1.7 * 1.7)}, &e, &s);
    REQUIRE(s == 0.0 && std::fabs(e - (0.25 + 0.3 - 1.7)) < 1e-15);
    std::printf("measure plan ok: %d cases\n", ncase);
    return 0;
}
