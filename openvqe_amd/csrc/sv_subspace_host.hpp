// sv_subspace_host.hpp — host-side plan of the subspace-expansion matrices S_ij = <phi_i|phi_j>, G_ij = <phi_i|H|phi_j>, phi_j = O_j psi
// (kernels: sv_subspace.hpp; handle section: subspace_host.inc; entry points ovqe_subspace_matrices / ovqe_subspace_info:
// abi_subspace.inc).  Host-only: no HIP, no handle types — g++ compiles it alone (tests/cpu/subspace_plan_check.cpp replays it the way
// the kernels index).  The functions marked OVQE_RDM_HD are the index arithmetic the kernels themselves run.
//
// ROWS.  R = { i : psi[i ^ x] != 0 for some distinct x mask of the pool }, a superset of every supp(phi_j): the bitmap of psi's support
// moved by every x (xor_word) and ORed, listed in ascending order.  The position of a register index in the list is the prefix count
// of its bitmap word plus the set bits of the word below it (row_position): no 2^n table.
// STORE.  Index-major like metric::Store, 16-byte amplitudes, row r = the r-th index of R:
//   columns [0, m) phi_j | zeros up to mb = m rounded up to the Gram block | columns [mb, mb + m) sigma_j = (H phi_j) on R | zeros
// wpad = 2 mb (mb when only S is asked for).
// GRAM.  Block pairs of 64 x 64 outputs: first the nb (nb + 1) / 2 pairs (I <= J < nb) of S in the order of rdm::block_pair (so that
// k_rdm_finish reads the slabs as they stand), then the nb * nb pairs (I < nb, J >= nb) of Phi^H Sigma.  No (Sigma, Sigma) pair.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "sv_rdm_host.hpp"

namespace ovqe {
namespace sub {

constexpr int SIGMA_GROUP_BATCH = 64;   // x-groups of H whose D_g(row) the 64 lanes of a wave compute side by side, then hand round
constexpr int SIGMA_ROW_TILE = 4;       // rows of one workgroup of the sigma kernel: one per wave
constexpr int SIGMA_THREADS = 64 * SIGMA_ROW_TILE;
constexpr int SIGMA_MAX_BLOCKS = 4;     // column blocks (of 64) a lane accumulates in registers; wider stores take several workgroups per row tile
constexpr int GRAM_TILE_ROWS = rdm::GRAM_TILE_BYTES / (rdm::GRAM_BLOCK * 16);   // rows of one staged tile of 16-byte amplitudes

// Dynamic LDS of k_sub_gram, one definition for kernel and host: [row tile of block I][row tile of block J]
struct GramLds { size_t b, bytes; };   // the tile of block I is at 0
OVQE_RDM_HD constexpr GramLds gram_lds() { return {(size_t)rdm::GRAM_TILE_BYTES, 2 * (size_t)rdm::GRAM_TILE_BYTES}; }

// word w of the bitmap `in` moved by x:  out[i] = in[i ^ x].  The bits of x below 6 permute inside the word (swaps of neighbouring runs
// of 1, 2, 4, 8, 16, 32 bits), the bits from 6 up choose the source word.  x < 2^n, so a register below 64 amplitudes stays inside its
// partial word.
OVQE_RDM_HD uint64_t xor_word(const uint64_t *in, uint64_t w, uint64_t x) {
    const uint64_t lowclear[6] = {0x5555555555555555ull, 0x3333333333333333ull, 0x0f0f0f0f0f0f0f0full,
                                  0x00ff00ff00ff00ffull, 0x0000ffff0000ffffull, 0x00000000ffffffffull};
    uint64_t v = in[w ^ (x >> 6)];
    for (int b = 0; b < 6; ++b)
        if ((x >> b) & 1u) v = ((v & lowclear[b]) << (1u << b)) | ((v >> (1u << b)) & lowclear[b]);
    return v;
}

OVQE_RDM_HD bool in_rows(const uint64_t *bitmap, uint64_t i) { return (bitmap[i >> 6] >> (i & 63u)) & 1u; }
// position of register index i (a set bit of the bitmap) in the ascending list; start = exclusive prefix sums of the words' popcounts
OVQE_RDM_HD uint64_t row_position(const uint64_t *bitmap, const uint64_t *start, uint64_t i) {
    const uint64_t below = bitmap[i >> 6] & ((1ull << (i & 63u)) - 1ull);
    return start[i >> 6] + (uint64_t)__builtin_popcountll(below);
}

// pair index -> (I, J) in units of column blocks of the STORE (block nb is the first block of Sigma)
OVQE_RDM_HD int s_pairs(int nb) { return nb * (nb + 1) / 2; }
OVQE_RDM_HD int total_pairs(int nb, bool with_h) { return s_pairs(nb) + (with_h ? nb * nb : 0); }
OVQE_RDM_HD void block_pair(int pair, int nb, int *I, int *J) {
    const int ns = s_pairs(nb);
    if (pair < ns) {
        rdm::block_pair(pair, nb, I, J);
    } else {
        const int q = pair - ns;
        *I = q / nb;
        *J = nb + (q - *I * nb);
    }
}
// the pair that holds output (block row I of Phi, block column J of Sigma), J counted from 0
OVQE_RDM_HD int h_pair_index(int I, int J, int nb) { return s_pairs(nb) + I * nb + J; }

struct Plan {
    int64_t rows = 0, m = 0, mb = 0, wpad = 0;
    bool with_h = false;
    int nb = 0, npairs = 0;          // column blocks of Phi, block pairs computed
    size_t store_bytes = 0;          // rows * wpad * 16
    int slices = 0;                  // row slices: one workgroup (and one slab) per (block pair, slice)
    int64_t slice_rows = 0;          // rows per slice (a multiple of GRAM_TILE_ROWS)
    size_t slab_elems = 0;           // npairs * slices * GRAM_BLOCK^2
    int sigma_blocks = 0;            // column blocks per lane of the sigma kernel (1, 2 or 4)
    int sigma_col_groups = 0;        // workgroups per row tile: nb / sigma_blocks rounded up
    int64_t sigma_row_tiles = 0;     // rows / SIGMA_ROW_TILE rounded up
};

// num_cus: the Gram grid aims at four workgroups per CU
inline Plan plan(int64_t rows, int64_t m, bool with_h, int num_cus) {
    Plan p;
    p.rows = rows;
    p.m = m;
    p.with_h = with_h;
    p.nb = (int)((m + rdm::GRAM_BLOCK - 1) / rdm::GRAM_BLOCK);
    p.mb = (int64_t)p.nb * rdm::GRAM_BLOCK;
    p.wpad = with_h ? 2 * p.mb : p.mb;
    p.npairs = total_pairs(p.nb, with_h);
    p.store_bytes = (size_t)rows * (size_t)p.wpad * 16u;
    const int64_t tiles = std::max<int64_t>(1, (rows + GRAM_TILE_ROWS - 1) / GRAM_TILE_ROWS);
    // (the slices are sized for the pairs of a call WITH h_out either way: S then has the same bits with and without it)
    const int64_t sized_for = total_pairs(p.nb, true);
    const int64_t want = ((int64_t)4 * std::max(num_cus, 1) + sized_for - 1) / sized_for;
    p.slices = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(want, tiles), rdm::GRAM_MAX_SLICES));
    p.slice_rows = (tiles + p.slices - 1) / p.slices * GRAM_TILE_ROWS;
    p.slices = (int)((tiles * GRAM_TILE_ROWS + p.slice_rows - 1) / p.slice_rows);   // no empty slice at the end
    p.slab_elems = (size_t)p.npairs * p.slices * rdm::GRAM_BLOCK * rdm::GRAM_BLOCK;
    p.sigma_blocks = p.nb >= SIGMA_MAX_BLOCKS ? SIGMA_MAX_BLOCKS : (p.nb >= 2 ? 2 : 1);
    p.sigma_col_groups = (p.nb + p.sigma_blocks - 1) / p.sigma_blocks;
    p.sigma_row_tiles = (rows + SIGMA_ROW_TILE - 1) / SIGMA_ROW_TILE;
    return p;
}

// the distinct x masks of a pool's terms, ascending
inline std::vector<uint64_t> distinct_x(const uint64_t *x, int64_t T) {
    std::vector<uint64_t> v(x, x + T);
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
    return v;
}

}  // namespace sub
}  // namespace ovqe
