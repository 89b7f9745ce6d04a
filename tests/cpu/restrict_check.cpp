// restrict_check.cpp — the restriction rule of openvqe_amd/csrc/sv_constrain_host.hpp (restrict_to_support: what build_sparse_program
// does to the Hamiltonian and constrain_host.inc to every observable) against entries the test derived from a DENSE restriction.
// Host only: g++ -fsanitize=address,undefined, no HIP (tests/test_constraint_cases.py builds and runs it).
//
//   restrict_check FILE      FILE: text, "ncases", then per case "m T E", m support states (18446744073709551615: a padding slot), T terms
//                            "x z c" (raw: the checker groups them as build_groups does — stable sort by x, i^ny folded in), E expected
//                            entries "i j c" in the rule's order.  Prints one line per case; exit status 1 on the first difference.
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <unordered_map>
#include <vector>

#include "../../openvqe_amd/csrc/sv_constrain_host.hpp"

using namespace ovqe;

int main(int argc, char **argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: restrict_check FILE\n");
        return 2;
    }
    std::FILE *f = std::fopen(argv[1], "r");
    if (!f) {
        std::fprintf(stderr, "cannot open %s\n", argv[1]);
        return 2;
    }
    int ncases = 0, status = 0;
    if (std::fscanf(f, "%d", &ncases) != 1) ncases = -1;
    for (int c = 0; c < ncases && !status; ++c) {
        int m = 0, T = 0, E = 0;
        if (std::fscanf(f, "%d %d %d", &m, &T, &E) != 3 || m < 0 || T < 0 || E < 0) {
            status = 2;
            break;
        }
        std::vector<uint64_t> support((size_t)m), x((size_t)T), z((size_t)T);
        std::vector<double> coeff((size_t)T);
        for (int k = 0; k < m; ++k)
            if (std::fscanf(f, "%" SCNu64, &support[(size_t)k]) != 1) status = 2;
        for (int t = 0; t < T; ++t)
            if (std::fscanf(f, "%" SCNu64 " %" SCNu64 " %lf", &x[(size_t)t], &z[(size_t)t], &coeff[(size_t)t]) != 3) status = 2;
        std::vector<uint32_t> wi((size_t)E), wj((size_t)E);
        std::vector<double> wc((size_t)E);
        for (int e = 0; e < E; ++e)
            if (std::fscanf(f, "%" SCNu32 " %" SCNu32 " %lf", &wi[(size_t)e], &wj[(size_t)e], &wc[(size_t)e]) != 3) status = 2;
        if (status) break;
        // the grouping of build_groups (ovqe_sv.hip)
        std::vector<int> order((size_t)T);
        std::iota(order.begin(), order.end(), 0);
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return x[(size_t)a] < x[(size_t)b]; });
        std::vector<HGroup> groups;
        std::vector<HTerm> terms;
        for (int oi = 0; oi < T; ++oi) {
            const size_t t = (size_t)order[(size_t)oi];
            HTerm ht;
            ht.z = z[t];
            fold_iny(coeff[t], 0.0, __builtin_popcountll(x[t] & z[t]), ht.cr, ht.ci);
            if (groups.empty() || x[(size_t)order[(size_t)oi - 1]] != x[t]) {
                HGroup g;
                g.x = x[t];
                g.jbase = 0;
                g.t0 = g.t1 = (int32_t)terms.size();
                g.tiny = 0.0;
                groups.push_back(g);
            }
            terms.push_back(ht);
            groups.back().t1 = (int32_t)terms.size();
        }
        std::unordered_map<uint64_t, int> index;
        for (int k = 0; k < m; ++k)
            if (support[(size_t)k] != ~0ull) index.emplace(support[(size_t)k], k);
        std::vector<SpEntry> got;
        const bool fits = constrain::restrict_to_support(groups, terms, support.data(), m, [&](uint64_t a) {
            auto it = index.find(a);
            return it == index.end() ? -1 : it->second;
        }, constrain::ENTRY_CAP, &got);
        if (!fits || got.size() != (size_t)E) {
            std::printf("case %d: %zu entries, expected %d\n", c, got.size(), E);
            status = 1;
            break;
        }
        for (int e = 0; e < E && !status; ++e) {
            const uint32_t gi = got[(size_t)e].ij & 0xfffu, gj = (got[(size_t)e].ij >> 12) & 0xfffu;
            if (gi != wi[(size_t)e] || gj != wj[(size_t)e] || got[(size_t)e].c != wc[(size_t)e] || got[(size_t)e].pad != 0) {
                std::printf("case %d entry %d: (%u, %u, %.17g), expected (%u, %u, %.17g)\n", c, e, gi, gj, got[(size_t)e].c, wi[(size_t)e],
                            wj[(size_t)e], wc[(size_t)e]);
                status = 1;
            }
        }
        if (!status) std::printf("case %d: m %d, %d terms in %zu groups, %d entries ok\n", c, m, T, groups.size(), E);
        // a cap below the entry count is reported, not overrun
        if (!status && E > 1) {
            std::vector<SpEntry> few;
            if (constrain::restrict_to_support(groups, terms, support.data(), m, [&](uint64_t a) {
                    auto it = index.find(a);
                    return it == index.end() ? -1 : it->second;
                }, (size_t)E - 1, &few) || few.size() != (size_t)E) {
                std::printf("case %d: the cap %d was not reported\n", c, E - 1);
                status = 1;
            }
        }
    }
    std::fclose(f);
    if (ncases < 0 || status == 2) {
        std::fprintf(stderr, "malformed input\n");
        return 2;
    }
    return status;
}
