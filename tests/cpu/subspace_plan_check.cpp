// subspace_plan_check.cpp — stand-alone replay of openvqe_amd/csrc/sv_subspace_host.hpp (g++ alone, run under ASan + UBSan by
// tests/test_subspace_cases.py): the bitmap arithmetic of the row set, the store layout, the block-pair list of the Gram kernel and
// the row schedules of the Gram and sigma kernels for random (rows, m), indexed the way the kernels index them.
//   usage: subspace_plan_check [seed]
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <utility>
#include <vector>

#include "../../openvqe_amd/csrc/sv_subspace_host.hpp"

using namespace ovqe;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            return 1;                                                      \
        }                                                                  \
    } while (0)

static int check_bitmaps(std::mt19937_64 &rng) {
    for (int n = 1; n <= 12; ++n)
        for (int rep = 0; rep < 6; ++rep) {
            const uint64_t namps = 1ull << n, nwords = rdm::bitmap_words(n);
            std::vector<uint64_t> in(nwords, 0), out(nwords, 0), start(nwords + 1, 0);
            std::vector<char> bit(namps, 0);
            for (uint64_t i = 0; i < namps; ++i)
                if (rng() % 3 == 0) {
                    bit[i] = 1;
                    in[i >> 6] |= 1ull << (i & 63);
                }
            // the image under a set of x masks, word by word, against the definition
            std::vector<uint64_t> xs;
            const int nx = 1 + (int)(rng() % 5);
            for (int k = 0; k < nx; ++k) xs.push_back(rng() & (namps - 1));
            if (rep == 0) xs[0] = 0;
            if (rep == 1) xs[0] = namps - 1;
            for (uint64_t w = 0; w < nwords; ++w)
                for (uint64_t x : xs) out[w] |= sub::xor_word(in.data(), w, x);
            std::vector<uint64_t> list;
            for (uint64_t i = 0; i < namps; ++i) {
                bool want = false;
                for (uint64_t x : xs) want = want || bit[i ^ x];
                CHECK(sub::in_rows(out.data(), i) == want);
                if (want) list.push_back(i);
            }
            if (n < 6) CHECK((out[0] >> namps) == 0);   // a partial word stays partial
            // positions from the prefix counts
            for (uint64_t w = 0; w < nwords; ++w) start[w + 1] = start[w] + (uint64_t)__builtin_popcountll(out[w]);
            CHECK(start[nwords] == list.size());
            for (size_t r = 0; r < list.size(); ++r) CHECK(sub::row_position(out.data(), start.data(), list[r]) == r);
        }
    const uint64_t xs[7] = {5, 0, 5, 9, 0, 1ull << 40, 9};
    const std::vector<uint64_t> d = sub::distinct_x(xs, 7);
    CHECK(d.size() == 4 && d[0] == 0 && d[1] == 5 && d[2] == 9 && d[3] == (1ull << 40));
    CHECK(sub::distinct_x(xs, 0).empty());
    return 0;
}

static int check_plan(int64_t rows, int64_t m, bool with_h, int cus) {
    const sub::Plan p = sub::plan(rows, m, with_h, cus);
    CHECK(p.rows == rows && p.m == m && p.with_h == with_h);
    CHECK(p.mb % rdm::GRAM_BLOCK == 0 && p.mb >= m && p.mb - m < rdm::GRAM_BLOCK && p.nb == p.mb / rdm::GRAM_BLOCK);
    CHECK(p.wpad == (with_h ? 2 * p.mb : p.mb));
    CHECK(p.store_bytes == (size_t)rows * (size_t)p.wpad * 16u);
    // ---- every block pair exactly once: (I <= J < nb) of S in the order k_rdm_finish reads, (I < nb, nb <= J < 2 nb) of Phi^H Sigma,
    // never a (Sigma, Sigma) pair, every column the pair reads inside the row
    const int nb = p.nb;
    CHECK(p.npairs == nb * (nb + 1) / 2 + (with_h ? nb * nb : 0));
    std::set<std::pair<int, int>> seen;
    for (int q = 0; q < p.npairs; ++q) {
        int I = -1, J = -1;
        sub::block_pair(q, nb, &I, &J);
        CHECK(I >= 0 && I < nb);            // the left factor is always a block of Phi
        CHECK(J >= I && J < (with_h ? 2 * nb : nb));
        CHECK(((int64_t)J + 1) * rdm::GRAM_BLOCK <= p.wpad);
        CHECK(seen.insert({I, J}).second);
        if (J < nb) CHECK(rdm::block_pair_index(I, J, nb) == q);
        else CHECK(sub::h_pair_index(I, J - nb, nb) == q);
    }
    for (int I = 0; I < nb; ++I) {
        for (int J = I; J < nb; ++J) CHECK(seen.count({I, J}) == 1);
        if (with_h)
            for (int J = nb; J < 2 * nb; ++J) CHECK(seen.count({I, J}) == 1);
    }
    CHECK((int)seen.size() == p.npairs);
    // ---- row slices of the Gram kernel: whole tiles, every row in exactly one slice, no empty slice (rows > 0)
    CHECK(p.slices >= 1 && p.slices <= rdm::GRAM_MAX_SLICES);
    CHECK(p.slice_rows > 0 && p.slice_rows % sub::GRAM_TILE_ROWS == 0);
    CHECK(sub::GRAM_TILE_ROWS * rdm::GRAM_BLOCK * 16 == rdm::GRAM_TILE_BYTES);
    CHECK(sub::gram_lds().bytes == 2u * rdm::GRAM_TILE_BYTES && sub::gram_lds().b == (size_t)rdm::GRAM_TILE_BYTES);
    int64_t covered = 0;
    for (int s = 0; s < p.slices; ++s) {
        const int64_t b = (int64_t)s * p.slice_rows, e = std::min(b + p.slice_rows, rows);
        if (rows > 0) CHECK(b < e);
        CHECK(b == covered || rows == 0);
        covered = std::max(covered, e);
    }
    CHECK(covered == rows);
    CHECK(p.slab_elems == (size_t)p.npairs * p.slices * rdm::GRAM_BLOCK * rdm::GRAM_BLOCK);
    // ---- the sigma kernel: column groups of sigma_blocks blocks cover the nb blocks, row tiles cover the rows
    CHECK(p.sigma_blocks == 1 || p.sigma_blocks == 2 || p.sigma_blocks == sub::SIGMA_MAX_BLOCKS);
    CHECK(p.sigma_col_groups * p.sigma_blocks >= nb && (p.sigma_col_groups - 1) * p.sigma_blocks < nb);
    CHECK(p.sigma_row_tiles * sub::SIGMA_ROW_TILE >= rows && (p.sigma_row_tiles - 1) * sub::SIGMA_ROW_TILE < std::max<int64_t>(rows, 1));
    CHECK(sub::SIGMA_THREADS == 64 * sub::SIGMA_ROW_TILE && sub::SIGMA_GROUP_BATCH == 64);
    return 0;
}

int main(int argc, char **argv) {
    const uint64_t seed = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1;
    std::mt19937_64 rng(seed);
    if (check_bitmaps(rng)) return 1;
    const int64_t edge_rows[] = {0, 1, 15, 16, 17, 4095, 4096, 4097}, edge_m[] = {1, 63, 64, 65, 128, 129, 256, 257, 700};
    for (int64_t rows : edge_rows)
        for (int64_t m : edge_m)
            for (int with_h = 0; with_h < 2; ++with_h)
                for (int cus : {0, 1, 256})
                    if (check_plan(rows, m, with_h != 0, cus)) return 1;
    for (int k = 0; k < 400; ++k) {
        const int64_t rows = (int64_t)(rng() % (k % 4 == 0 ? 3000000 : 5000));
        const int64_t m = 1 + (int64_t)(rng() % (k % 3 == 0 ? 1500 : 200));
        if (check_plan(rows, m, rng() & 1, (int)(rng() % 400))) return 1;
    }
    std::printf("subspace plan ok\n");
    return 0;
}
