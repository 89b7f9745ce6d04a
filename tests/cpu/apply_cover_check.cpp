// apply_cover_check.cpp — the cover rule of the Pauli-sum application (grow_tile_set, openvqe_amd/csrc/sv_cover_host.hpp) compiled alone
// with g++ (ASan + UBSan in tests/test_stream_cases.py), driven the way build_ham_tiles (tile_host.inc) drives it on a complex register.
//   usage: apply_cover_check FILE      FILE: one case per line, "n M low G x_0 ... x_(G-1)" — the distinct x masks of a Hamiltonian
// Per case: the groups whose x mask with the `low` forced bits exceeds M bits are the untiled rest; the others, in ascending order of x,
// are covered by sets grown from the low bits until none is left.  Printed for the test to compare with its Python restatement
// (tests/stream_cases.py: apply_cover): "case sweeps=<k> rest=<r> S_0 ... S_(k-1)".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../openvqe_amd/csrc/sv_cover_host.hpp"

using namespace ovqe;

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::FILE *f = std::fopen(argv[1], "r");
    if (!f) return 2;
    int n = 0, M = 0, low = 0, G = 0, cases = 0;
    while (std::fscanf(f, "%d %d %d %d", &n, &M, &low, &G) == 4) {
        std::vector<uint64_t> xs((size_t)G);
        for (uint64_t &x : xs) {
            unsigned long long v = 0;
            if (std::fscanf(f, "%llu", &v) != 1) return 2;
            x = v;
        }
        std::sort(xs.begin(), xs.end());
        const uint64_t lowbits = (1ull << low) - 1ull;
        std::vector<uint64_t> left, sweeps;
        int rest = 0;
        for (const uint64_t x : xs) {
            if (__builtin_popcountll(x | lowbits) > M) ++rest;
            else left.push_back(x);
        }
        while (!left.empty()) {
            const uint64_t S = grow_tile_set(left, lowbits, M, n);
            if (__builtin_popcountll(S) != M || (S & lowbits) != lowbits || (n < 64 && (S >> n))) {
                std::printf("FAIL: S = %llx is not %d bits of the lowest %d with the low bits\n", (unsigned long long)S, M, n);
                return 1;
            }
            std::vector<uint64_t> next;
            for (const uint64_t x : left)
                if (x & ~S) next.push_back(x);
            if (next.size() == left.size()) {
                std::printf("FAIL: a sweep that takes no group\n");
                return 1;
            }
            left.swap(next);
            sweeps.push_back(S);
        }
        std::printf("case sweeps=%zu rest=%d", sweeps.size(), rest);
        for (const uint64_t S : sweeps) std::printf(" %llu", (unsigned long long)S);
        std::printf("\n");
        ++cases;
    }
    std::fclose(f);
    std::printf("apply cover ok (%d cases)\n", cases);
    return 0;
}
