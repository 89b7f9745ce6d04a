// sv_rdm_host.hpp — host-side plan of the one- and two-particle density matrices of the resident state (kernels: sv_rdm.hpp; handle
// section: rdm_host.inc; entry points ovqe_rdm / ovqe_rdm_info: abi_rdm.inc).  Host-only: no HIP, no handle types — g++ compiles it
// alone (tests/cpu/rdm_plan_check.cpp replays it the way the kernels index).  The functions marked OVQE_RDM_HD are the index
// arithmetic the kernels themselves run: the device code calls these very definitions.
//
// Jordan-Wigner, orbital p = reference qubit p = index bit n-1-p.  For a register index K (an occupation pattern):
//   order 1:  v_K[a]     = (-1)^{occ_K(t < a)}     psi[K | bit(a)]            a not in K
//   order 2:  v_K[(a<b)] = (-1)^{occ_K(a < t < b)} psi[K | bit(a) | bit(b)]   a, b not in K     (pairs in lexicographic order)
// and gamma = sum_K conj(v_K) v_K^T, D2 likewise: Gram matrices over the ROWS K that lie one / two annihilations below a non-zero
// amplitude.  The rows come from a bitmap of the support (census), its down-shadow(s), and the ascending list of the shadow's bits.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define OVQE_RDM_HD __host__ __device__ inline
#else
#define OVQE_RDM_HD inline
#endif

namespace ovqe {
namespace rdm {

constexpr int GRAM_BLOCK = 64;       // columns of one block of the Gram matrix: a workgroup computes GRAM_BLOCK x GRAM_BLOCK outputs
constexpr int GRAM_THREADS = 256;    // 16 x 16 threads, a 4 x 4 register tile each
constexpr int GRAM_TILE_BYTES = 16384;   // bytes of one staged row tile of one column block (rows x GRAM_BLOCK elements)
constexpr int GRAM_MAX_SLICES = 256;
constexpr int TIMED_CHUNKS_MAX = 64;     // the per-kernel times are kept for calls of at most this many row chunks

struct ColEntry {      // one column of a row: the bits it adds to K, the bits whose occupation gives the sign
    uint64_t add, between;
};

OVQE_RDM_HD int64_t width(int n, int order) { return order == 1 ? (int64_t)n : (int64_t)n * (n - 1) / 2; }
OVQE_RDM_HD uint64_t orbital_bit(int n, int a) { return 1ull << (n - 1 - a); }

// the column table: order 1 n entries, order 2 n (n - 1) / 2 entries, pairs (a < b) in lexicographic order
inline void build_columns(int n, int order, std::vector<ColEntry> &cols) {
    cols.clear();
    const uint64_t all = n >= 64 ? ~0ull : ((1ull << n) - 1ull);
    if (order == 1) {
        for (int a = 0; a < n; ++a) {
            const uint64_t ba = orbital_bit(n, a);
            cols.push_back(ColEntry{ba, all & ~((ba << 1) - 1ull)});   // orbitals t < a: the index bits above bit(a)
        }
    } else {
        for (int a = 0; a < n; ++a)
            for (int b = a + 1; b < n; ++b) {
                const uint64_t ba = orbital_bit(n, a), bb = orbital_bit(n, b);
                cols.push_back(ColEntry{ba | bb, (ba - 1ull) & ~((bb << 1) - 1ull)});   // a < t < b: strictly between the two bits
            }
    }
}

// one element of a row: the gather index (or ~0: an orbital of the column is occupied in K, the entry is zero) and the sign
OVQE_RDM_HD uint64_t column_source(uint64_t K, ColEntry c, bool *negative) {
    *negative = (__builtin_popcountll(K & c.between) & 1) != 0;
    return (K & c.add) ? ~0ull : (K | c.add);
}

// ---- bitmaps: bit D of word D >> 6.  A register below 64 amplitudes is one partial word (bits from 2^n on are zero).
OVQE_RDM_HD uint64_t bitmap_words(int n) { return n <= 6 ? 1ull : (1ull << (n - 6)); }

// word w of the down-shadow of `in`:  out[K] = OR over the orbitals a not in K of in[K | bit(a)].  Index bits below 6 move inside the
// word (a masked shift), bits from 6 up pair word w with word w | stride.
OVQE_RDM_HD uint64_t shadow_word(const uint64_t *in, uint64_t w, int n) {
    const uint64_t lowclear[6] = {0x5555555555555555ull, 0x3333333333333333ull, 0x0f0f0f0f0f0f0f0full,
                                  0x00ff00ff00ff00ffull, 0x0000ffff0000ffffull, 0x00000000ffffffffull};
    const uint64_t own = in[w];
    uint64_t out = 0;
    for (int b = 0; b < 6 && b < n; ++b) out |= (own >> (1u << b)) & lowclear[b];
    for (int b = 6; b < n; ++b) {
        const uint64_t stride = 1ull << (b - 6);
        if (!(w & stride)) out |= in[w | stride];
    }
    return out;
}

// ---- schedule of the Gram kernel
// Upper-triangular block pairs (I <= J) in row-major order of I: pair index -> (I, J)
OVQE_RDM_HD void block_pair(int pair, int nblk, int *I, int *J) {
    int i = 0, left = pair;
    while (left >= nblk - i) {
        left -= nblk - i;
        ++i;
    }
    *I = i;
    *J = i + left;
}
OVQE_RDM_HD int block_pair_index(int I, int J, int nblk) { return I * nblk - I * (I - 1) / 2 + (J - I); }

// the four columns (of the 64 of a block) thread coordinate t = 0..15 owns, j = 0..3: chosen so that the 16 lanes that differ in t read
// 16 consecutive 16-byte slots of the staged row (8-byte elements: two columns per slot, 16-byte elements: one)
OVQE_RDM_HD int owned_column(bool real, int t, int j) { return real ? (j >> 1) * 32 + t * 2 + (j & 1) : j * 16 + t; }

struct Schedule {
    int order = 0, n = 0;
    bool real = false;
    int64_t width = 0, wpad = 0;     // columns of a row, padded to the Gram block
    int nblk = 0, npairs = 0;        // column blocks, block pairs (I <= J)
    int tile_rows = 0;               // rows of one staged tile
    size_t elem_bytes = 0, row_bytes = 0;
    int64_t rows = 0;
    int64_t chunk_rows = 0;          // rows per workspace chunk (a multiple of tile_rows)
    int64_t nchunks = 0;
    int slices = 0;                  // row slices of a chunk: one workgroup (and one partial slab) per (block pair, slice)
    int64_t slice_rows = 0;          // rows per slice (a multiple of tile_rows)
    size_t workspace_bytes = 0;      // chunk_rows * row_bytes
    size_t slab_elems = 0;           // elements of all partial slabs: npairs * slices * GRAM_BLOCK^2
};

// workspace_mb: option "rdm_workspace_mb" (the minimum is one staging tile); num_cus: the grid aims at four workgroups per CU
inline Schedule plan(int n, int order, bool real, int64_t rows, int64_t workspace_mb, int num_cus) {
    Schedule s;
    s.order = order;
    s.n = n;
    s.real = real;
    s.width = width(n, order);
    s.nblk = (int)((s.width + GRAM_BLOCK - 1) / GRAM_BLOCK);
    s.wpad = (int64_t)s.nblk * GRAM_BLOCK;
    s.npairs = s.nblk * (s.nblk + 1) / 2;
    s.elem_bytes = real ? 8 : 16;
    s.row_bytes = (size_t)s.wpad * s.elem_bytes;
    s.tile_rows = (int)(GRAM_TILE_BYTES / (GRAM_BLOCK * s.elem_bytes));
    s.rows = rows;
    const int64_t need = std::max<int64_t>(1, (rows + s.tile_rows - 1) / s.tile_rows) * s.tile_rows;
    const int64_t fit = (int64_t)(((size_t)std::max<int64_t>(workspace_mb, 0) << 20) / s.row_bytes) / s.tile_rows * s.tile_rows;
    s.chunk_rows = std::min(need, std::max<int64_t>(fit, s.tile_rows));
    s.nchunks = rows > 0 ? (rows + s.chunk_rows - 1) / s.chunk_rows : 0;
    const int64_t tiles = s.chunk_rows / s.tile_rows;
    const int64_t want = ((int64_t)4 * std::max(num_cus, 1) + s.npairs - 1) / s.npairs;
    s.slices = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(want, tiles), GRAM_MAX_SLICES));
    s.slice_rows = (tiles + s.slices - 1) / s.slices * s.tile_rows;
    s.slices = (int)((s.chunk_rows + s.slice_rows - 1) / s.slice_rows);   // no empty slice at the end
    s.workspace_bytes = (size_t)s.chunk_rows * s.row_bytes;
    s.slab_elems = (size_t)s.npairs * s.slices * GRAM_BLOCK * GRAM_BLOCK;
    return s;
}

}  // namespace rdm
}  // namespace ovqe
