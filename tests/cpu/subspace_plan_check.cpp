// subspace_plan_check.cpp — stand-alone replay of openvqe_amd/csrc/sv_subspace_host.hpp (g++ alone, run under ASan + UBSan by
// tests/test_subspace_cases.py): the bitmap arithmetic of the row set, the store layout, the block-pair list of the Gram kernel and
// the row schedules of the Gram and sigma kernels for random (rows, m), indexed the way the kernels index them.
//   usage: subspace_plan_check [seed]
//          subspace_plan_check boundary rows,m,with_h,cus ...     the plan of each tuple, printed, with every row placed in its
//                                                                 (slice, tile) and every column block in its (column group, b), then
//                                                                 the pair lists at nb = 4, 5, 6 and the bitmap words of 1 .. 5 qubits
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

// ---- boundary mode ------------------------------------------------------------------------------------------------------------------------
// every row in exactly one (slice, tile) the way k_sub_gram walks them, no slice without rows; every column block in exactly one
// (column group, b) with blk0 + b < nb the way k_sub_sigma walks them; every row in exactly one pass of a strided sigma grid
static int check_boundary_tuple(int64_t rows, int64_t m, bool with_h, int cus) {
    if (check_plan(rows, m, with_h, cus)) return 1;
    const sub::Plan p = sub::plan(rows, m, with_h, cus);
    std::printf("plan rows=%lld m=%lld with_h=%d cus=%d nb=%d mb=%lld wpad=%lld pairs=%d slices=%d slice_rows=%lld sigma_blocks=%d col_groups=%d row_tiles=%lld\n",
                (long long)rows, (long long)m, with_h ? 1 : 0, cus, p.nb, (long long)p.mb, (long long)p.wpad, p.npairs, p.slices,
                (long long)p.slice_rows, p.sigma_blocks, p.sigma_col_groups, (long long)p.sigma_row_tiles);
    std::vector<unsigned char> hits((size_t)rows, 0);
    constexpr int TR = sub::GRAM_TILE_ROWS;
    for (int s = 0; s < p.slices; ++s) {
        const int64_t r_begin = (int64_t)s * p.slice_rows;
        const int64_t r_end = r_begin + p.slice_rows < rows ? r_begin + p.slice_rows : rows;
        if (rows > 0) CHECK(r_begin < r_end);
        for (int64_t r0 = r_begin; r0 < r_end; r0 += TR)
            for (int row = 0; row < TR; ++row)
                if (r0 + row < r_end) {
                    CHECK(r0 + row < rows);
                    CHECK(++hits[(size_t)(r0 + row)] == 1);
                }
    }
    for (int64_t r = 0; r < rows; ++r) CHECK(hits[(size_t)r] == 1);
    std::vector<int> blocks((size_t)p.nb, 0);
    for (int g = 0; g < p.sigma_col_groups; ++g) {
        int live = 0;
        for (int b = 0; b < p.sigma_blocks; ++b)
            if (g * p.sigma_blocks + b < p.nb) {
                CHECK(((int64_t)(g * p.sigma_blocks + b) + 1) * 64 <= p.mb);
                ++blocks[(size_t)(g * p.sigma_blocks + b)];
                ++live;
            }
        CHECK(live >= 1);   // no column group without a block
    }
    for (int b = 0; b < p.nb; ++b) CHECK(blocks[(size_t)b] == 1);
    // the strided row loop of the sigma kernel on a grid of min(row tiles, 32 cus) workgroups of SIGMA_ROW_TILE waves
    const int64_t gx = std::min<int64_t>(p.sigma_row_tiles, (int64_t)std::max(cus, 1) * 32);
    std::fill(hits.begin(), hits.end(), 0);
    for (int64_t blk = 0; blk < gx; ++blk)
        for (int wave = 0; wave < sub::SIGMA_ROW_TILE; ++wave)
            for (int64_t r = blk * sub::SIGMA_ROW_TILE + wave; r < rows; r += gx * sub::SIGMA_ROW_TILE) CHECK(++hits[(size_t)r] == 1);
    for (int64_t r = 0; r < rows; ++r) CHECK(hits[(size_t)r] == 1);
    return 0;
}

static int check_pair_lists() {
    for (int nb = 4; nb <= 6; ++nb) {
        const int ns = sub::s_pairs(nb);
        CHECK(sub::total_pairs(nb, true) == ns + nb * nb && sub::total_pairs(nb, false) == ns);
        for (int q = 0; q < sub::total_pairs(nb, true); ++q) {
            int I = -1, J = -1;
            sub::block_pair(q, nb, &I, &J);
            if (q < ns) CHECK(0 <= I && I <= J && J < nb && rdm::block_pair_index(I, J, nb) == q);
            else CHECK(0 <= I && I < nb && nb <= J && J < 2 * nb && sub::h_pair_index(I, J - nb, nb) == q);
        }
        for (int I = 0; I < nb; ++I)
            for (int J = 0; J < nb; ++J) {
                int I2 = -1, J2 = -1;
                sub::block_pair(sub::h_pair_index(I, J, nb), nb, &I2, &J2);
                CHECK(I2 == I && J2 == nb + J);
            }
    }
    return 0;
}

// xor_word and row_position on the one partial word of 1 .. 5 qubits against the definition, for every x: every bitmap up to 3 qubits,
// the empty, full, one-bit and 300 random bitmaps on 4 and 5
static int check_partial_words() {
    std::mt19937_64 rng(5);
    for (int n = 1; n <= 5; ++n) {
        const uint64_t namps = 1ull << n, full = namps == 64 ? ~0ull : (1ull << namps) - 1ull;
        CHECK(rdm::bitmap_words(n) == 1);
        std::vector<uint64_t> maps;
        if (n <= 3) {
            for (uint64_t v = 0; v <= full; ++v) maps.push_back(v);
        } else {
            maps.push_back(0);
            maps.push_back(full);
            for (uint64_t i = 0; i < namps; ++i) maps.push_back(1ull << i);
            for (int k = 0; k < 300; ++k) maps.push_back(rng() & full);
        }
        for (uint64_t in : maps)
            for (uint64_t x = 0; x < namps; ++x) {
                const uint64_t out = sub::xor_word(&in, 0, x);
                uint64_t want = 0;
                for (uint64_t i = 0; i < namps; ++i)
                    if ((in >> (i ^ x)) & 1u) want |= 1ull << i;
                CHECK(out == want);
                CHECK((out & ~full) == 0);
                const uint64_t start[2] = {0, (uint64_t)__builtin_popcountll(out)};
                uint64_t r = 0;
                for (uint64_t i = 0; i < namps; ++i)
                    if (sub::in_rows(&out, i)) CHECK(sub::row_position(&out, start, i) == r++);
                CHECK(r == start[1]);
            }
    }
    return 0;
}

static int boundary(int argc, char **argv) {
    for (int a = 2; a < argc; ++a) {
        long long rows = -1, m = -1;
        int with_h = -1, cus = -1;
        if (std::sscanf(argv[a], "%lld,%lld,%d,%d", &rows, &m, &with_h, &cus) != 4 || rows < 0 || m < 1 || with_h < 0 || with_h > 1 || cus < 0) {
            std::printf("FAILED: bad tuple '%s' (rows,m,with_h,cus)\n", argv[a]);
            return 1;
        }
        if (check_boundary_tuple(rows, m, with_h != 0, cus)) return 1;
    }
    if (check_pair_lists()) return 1;
    if (check_partial_words()) return 1;
    std::printf("subspace boundary ok\n");
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && std::strcmp(argv[1], "boundary") == 0) return boundary(argc, argv);
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
