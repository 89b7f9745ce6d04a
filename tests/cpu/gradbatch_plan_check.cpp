// gradbatch_plan_check.cpp — the launch planner of the batched exact gradient (openvqe_amd/csrc/sv_gradbatch_host.hpp) and the kernel's
// LDS layout (sp_grad_batch_lds, sv_sparse_layout.hpp) compiled alone with g++ (ASan + UBSan in tests/test_gradbatch_cases.py).
//   usage: gradbatch_plan_check FILE      FILE: one case per line, "m ntab nops npairs K B waves workgroups cus"
// For every case the layout's regions are checked (16-byte strides, private regions that do not overlap, the shared tables behind the
// last wave, every row of the batch owned by exactly one wave) and the planner's choice is printed for the test to compare with its
// Python restatement (tests/gradbatch_cases.py).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../openvqe_amd/csrc/sv_gradbatch_host.hpp"

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
    const SpGradBatchLds L = sp_grad_batch_lds(A, nw, stage);
    const SpGradLds W = sp_grad_lds(A, false);
    CHECK(L.stride % 16 == 0 && L.stride >= W.bytes && L.stride < W.bytes + 16, "stride %zu of a region of %zu bytes", L.stride, W.bytes);
    CHECK(L.lam == (size_t)A.mpad * 8 && L.cs == 2 * L.lam && L.cs % 16 == 0, "vector regions");
    CHECK(L.w == L.cs + (size_t)A.ntab * 16 && L.gk == L.w + (size_t)A.ntab * 8 && L.gk + (size_t)A.K * 8 <= L.stride, "table regions");
    CHECK(L.ops == (size_t)nw * L.stride && L.ops % 16 == 0 && L.pairs == L.ops + (size_t)A.nops * 16, "shared tables behind the last wave");
    CHECK(L.bytes == (stage ? L.pairs + (size_t)A.npairs * 4 : L.ops), "bytes");
}

// every row b < B is visited once, by wave (b / nw) % grid ... of the kernel's loop: b = g nw + v, += grid nw
static void check_rows(int64_t B, int nw, int64_t grid) {
    if (B > 4096) return;
    std::vector<int> seen((size_t)B, 0);
    for (int64_t g = 0; g < grid; ++g)
        for (int v = 0; v < nw; ++v)
            for (int64_t b = g * nw + v; b < B; b += grid * nw) ++seen[(size_t)b];
    for (int64_t b = 0; b < B; ++b) CHECK(seen[(size_t)b] == 1, "row %lld visited %d times (B %lld, nw %d, grid %lld)", (long long)b, seen[(size_t)b], (long long)B, nw, (long long)grid);
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::FILE *f = std::fopen(argv[1], "r");
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
        const gradbatch::Plan P = gradbatch::plan(A, A.B, (int)v[6], v[7], (int)v[8]);
        CHECK(P.ok == gradbatch::eligible(A), "a plan exactly for the eligible programs");
        if (P.ok) {
            CHECK(P.lds == sp_grad_batch_lds(A, P.nw, P.stage).bytes && P.lds <= gradbatch::LDS_BUDGET, "the launch exceeds the budget");
            CHECK(P.per_cu >= 1 && (size_t)P.per_cu * P.lds <= gradbatch::LDS_CU && P.per_cu * P.nw <= gradbatch::waves_cu(P.stage), "residency");
            CHECK(P.workgroups >= 1 && (P.workgroups - 1) * P.nw < std::max<int64_t>(A.B, 1), "a workgroup without a row");
            CHECK(v[7] <= 0 || P.workgroups <= v[7], "the cap on the grid");
            check_rows(A.B, P.nw, P.workgroups);
        }
        std::printf("case m=%d ntab=%d nops=%d npairs=%d K=%d B=%lld waves=%lld cap=%lld cus=%lld eligible=%d ok=%d nw=%d stage=%d per_cu=%d workgroups=%lld lds=%zu\n",
                    A.m, A.ntab, A.nops, A.npairs, A.K, v[5], v[6], v[7], v[8], (int)gradbatch::eligible(A), (int)P.ok, P.nw, (int)P.stage, P.per_cu,
                    (long long)P.workgroups, P.lds);
        ++cases;
    }
    std::fclose(f);
    if (fails) {
        std::printf("gradbatch plan: %d failures\n", fails);
        return 1;
    }
    std::printf("gradbatch plan ok (%d cases)\n", cases);
    return 0;
}
