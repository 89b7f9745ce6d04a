// sv_rdm.hpp — kernels of the one- and two-particle density matrices of the resident state (plan and index arithmetic:
// sv_rdm_host.hpp; launches: rdm_host.inc).  The state buffer is only read.  No atomics: every partial sum has one owner and the
// slabs are reduced in a fixed order, so a call gives the same bits every time.
//   k_rdm_census       bitmap of the support (64-lane ballot, one 8-byte store per wave), non-zero count, "some imaginary part" flag
//   k_rdm_shadow       down-shadow of a bitmap, all orbitals in one pass (the bitmap is 2^n / 8 bytes: cache-resident)
//   k_rdm_popc / k_rdm_list   popcounts of the shadow's words (their prefix sums: rocprim), the set bits in ascending order
//   k_rdm_rows         V[row][column] of a chunk of rows: one gather from psi and one popcount parity per element
//   k_rdm_gram         partial Gram matrices V^H V per (block pair I <= J, row slice), 4 x 4 fp64 accumulators per thread
//   k_rdm_finish       sum of the slabs in slice order, Hermitian mirror, the packed result
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sv_kernels.hpp"
#include "sv_rdm_host.hpp"

namespace ovqe {

// ---- census: one word of the bitmap per wave and step, grid-stride over the words.  census[block] = (non-zero amplitudes, 1 when one
// of them has an imaginary part).
__global__ __launch_bounds__(256) void k_rdm_census(const amp_t *__restrict__ st, uint64_t namps, uint64_t nwords,
                                                    uint64_t *__restrict__ bitmap, ulonglong2 *__restrict__ census) {
    __shared__ uint64_t s_cnt[4], s_im[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const v2d *p = reinterpret_cast<const v2d *>(st);
    uint64_t cnt = 0, im = 0;
    for (uint64_t w = (uint64_t)blockIdx.x * 4u + wave; w < nwords; w += (uint64_t)gridDim.x * 4u) {
        const uint64_t i = w * 64u + lane;
        v2d a = {0.0, 0.0};
        if (i < namps) a = p[i];
        const uint64_t nz = __ballot(a.x != 0.0 || a.y != 0.0);
        const uint64_t ni = __ballot(a.y != 0.0);
        if (lane == 0) bitmap[w] = nz;
        cnt += __builtin_popcountll(nz);
        im |= ni;
    }
    if (lane == 0) {
        s_cnt[wave] = cnt;
        s_im[wave] = im;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        ulonglong2 r;
        r.x = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        r.y = (s_im[0] | s_im[1] | s_im[2] | s_im[3]) ? 1ull : 0ull;
        census[blockIdx.x] = r;
    }
}

__global__ __launch_bounds__(256) void k_rdm_shadow(const uint64_t *__restrict__ in, uint64_t *__restrict__ out, uint64_t nwords, int n) {
    const uint64_t w = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (w < nwords) out[w] = rdm::shadow_word(in, w, n);
}

// counts[w] = set bits of word w, counts[nwords] = 0: the exclusive prefix sums of nwords + 1 entries end with the total
__global__ __launch_bounds__(256) void k_rdm_popc(const uint64_t *__restrict__ bitmap, uint64_t nwords, uint64_t *__restrict__ counts) {
    const uint64_t w = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (w <= nwords) counts[w] = w < nwords ? (uint64_t)__builtin_popcountll(bitmap[w]) : 0ull;
}

__global__ __launch_bounds__(256) void k_rdm_list(const uint64_t *__restrict__ bitmap, uint64_t nwords, const uint64_t *__restrict__ start,
                                                  uint64_t *__restrict__ rows) {
    const uint64_t w = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (w >= nwords) return;
    uint64_t m = bitmap[w], at = start[w];
    while (m) {
        rows[at++] = w * 64u + (uint64_t)__builtin_ctzll(m);
        m &= m - 1;
    }
}

// ---- rows: element e of the chunk is (row e / wpad, column e % wpad); wpad is a multiple of 64, so a wave holds 64 consecutive columns
// of ONE row and its stores are one contiguous run.  Columns from `width` on are zero.
template <bool REAL>
__global__ __launch_bounds__(256) void k_rdm_rows(const amp_t *__restrict__ st, const uint64_t *__restrict__ rows, int64_t nrows,
                                                  const rdm::ColEntry *__restrict__ cols, int64_t width, int64_t wpad, void *__restrict__ out) {
    const uint64_t total = (uint64_t)nrows * (uint64_t)wpad;
    for (uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x; e < total; e += (uint64_t)gridDim.x * 256u) {
        const uint64_t r = e / (uint64_t)wpad;
        const int64_t c = (int64_t)(e - r * (uint64_t)wpad);
        v2d v = {0.0, 0.0};
        if (c < width) {
            const uint64_t K = rows[r];
            bool neg;
            const uint64_t src = rdm::column_source(K, cols[c], &neg);
            if (src != ~0ull) {
                const v2d a = reinterpret_cast<const v2d *>(st)[src];
                v = neg ? -a : a;
            }
        }
        if (REAL) reinterpret_cast<double *>(out)[e] = v.x;
        else reinterpret_cast<v2d *>(out)[e] = v;
    }
}

// ---- Gram.  Dynamic LDS of k_rdm_gram, one definition for kernel and host: [row tile of block I][row tile of block J]
struct RdmGramLds { size_t b, bytes; };   // the tile of block I is at 0
__host__ __device__ constexpr RdmGramLds rdm_gram_lds() { return {(size_t)rdm::GRAM_TILE_BYTES, 2 * (size_t)rdm::GRAM_TILE_BYTES}; }

// Workgroup blockIdx.x = pair * slices + slice: G[p][q] += sum over the slice's rows of conj(V[row][I * 64 + p]) V[row][J * 64 + q] into
// its own slab of 64 x 64 elements.  Thread (ty, tx) of 16 x 16 owns rows rdm::owned_column(ty, i) and columns rdm::owned_column(tx, j).
template <bool REAL>
__global__ __launch_bounds__(rdm::GRAM_THREADS) void k_rdm_gram(const void *__restrict__ V, int64_t nrows, int64_t wpad, int nblk, int slices,
                                                                int64_t slice_rows, void *__restrict__ slabs) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int ES = REAL ? 8 : 16;                                  // bytes of an element
    constexpr int TR = rdm::GRAM_TILE_BYTES / (rdm::GRAM_BLOCK * ES);  // rows of a tile
    constexpr int UPR = rdm::GRAM_BLOCK * ES / 16;                     // 16-byte units of one row of a block
    constexpr int UNITS = rdm::GRAM_TILE_BYTES / 16 / rdm::GRAM_THREADS;   // units a thread stages per tile
    constexpr RdmGramLds L = rdm_gram_lds();
    v2d *la = reinterpret_cast<v2d *>(smem);
    v2d *lb = reinterpret_cast<v2d *>(smem + L.b);
    const int pair = blockIdx.x / slices, slice = blockIdx.x - pair * slices;
    const int64_t r_begin = (int64_t)slice * slice_rows;
    const int64_t r_end = r_begin + slice_rows < nrows ? r_begin + slice_rows : nrows;
    if (r_begin >= r_end) return;   // (an empty slice of the last chunk: its slab keeps what it has)
    int I, J;
    rdm::block_pair(pair, nblk, &I, &J);
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const size_t row_bytes = (size_t)wpad * ES;
    const unsigned char *base = reinterpret_cast<const unsigned char *>(V);
    double acc_re[4][4], acc_im[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc_re[i][j] = acc_im[i][j] = 0.0;
    for (int64_t r0 = r_begin; r0 < r_end; r0 += TR) {
        v2d ga[UNITS], gb[UNITS];
#pragma unroll
        for (int u = 0; u < UNITS; ++u) {
            const int unit = threadIdx.x + u * rdm::GRAM_THREADS;
            const int row = unit / UPR, cu = unit - row * UPR;
            ga[u] = gb[u] = v2d{0.0, 0.0};
            if (r0 + row < r_end) {
                const unsigned char *src = base + (size_t)(r0 + row) * row_bytes;
                ga[u] = reinterpret_cast<const v2d *>(src + (size_t)I * rdm::GRAM_BLOCK * ES)[cu];
                gb[u] = reinterpret_cast<const v2d *>(src + (size_t)J * rdm::GRAM_BLOCK * ES)[cu];
            }
        }
        __syncthreads();   // the previous tile has been read
#pragma unroll
        for (int u = 0; u < UNITS; ++u) {
            const int unit = threadIdx.x + u * rdm::GRAM_THREADS;
            la[unit] = ga[u];
            lb[unit] = gb[u];
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < TR; ++k) {
            if (REAL) {
                const v2d a01 = la[k * UPR + ty], a23 = la[k * UPR + 16 + ty];
                const v2d b01 = lb[k * UPR + tx], b23 = lb[k * UPR + 16 + tx];
                const double a[4] = {a01.x, a01.y, a23.x, a23.y}, b[4] = {b01.x, b01.y, b23.x, b23.y};
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc_re[i][j] = fma(a[i], b[j], acc_re[i][j]);
            } else {
                v2d a[4], b[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    a[i] = la[k * UPR + i * 16 + ty];
                    b[i] = lb[k * UPR + i * 16 + tx];
                }
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {   // conj(a) b
                        acc_re[i][j] = fma(a[i].y, b[j].y, fma(a[i].x, b[j].x, acc_re[i][j]));
                        acc_im[i][j] = fma(-a[i].y, b[j].x, fma(a[i].x, b[j].y, acc_im[i][j]));
                    }
            }
        }
    }
    const size_t slab = (size_t)blockIdx.x * rdm::GRAM_BLOCK * rdm::GRAM_BLOCK;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const size_t at = slab + (size_t)rdm::owned_column(REAL, ty, i) * rdm::GRAM_BLOCK + rdm::owned_column(REAL, tx, j);
            if (REAL) {
                reinterpret_cast<double *>(slabs)[at] += acc_re[i][j];
            } else {
                v2d *o = reinterpret_cast<v2d *>(slabs) + at;
                *o += v2d{acc_re[i][j], acc_im[i][j]};
            }
        }
}

// out[p][q] (W x W complex, row-major) for p <= q from the slabs of block pair (p / 64, q / 64) summed in slice order; out[q][p] is its
// conjugate and the diagonal is real: the result is Hermitian to the bit
template <bool REAL>
__global__ __launch_bounds__(256) void k_rdm_finish(const void *__restrict__ slabs, int64_t W, int nblk, int slices, double2 *__restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= W * W) return;
    const int64_t p = e / W, q = e - p * W;
    if (p > q) return;
    const int I = (int)(p / rdm::GRAM_BLOCK), J = (int)(q / rdm::GRAM_BLOCK);
    const size_t first = (size_t)rdm::block_pair_index(I, J, nblk) * slices * rdm::GRAM_BLOCK * rdm::GRAM_BLOCK +
                         (size_t)(p - (int64_t)I * rdm::GRAM_BLOCK) * rdm::GRAM_BLOCK + (size_t)(q - (int64_t)J * rdm::GRAM_BLOCK);
    double re = 0.0, im = 0.0;
    for (int s = 0; s < slices; ++s) {
        const size_t at = first + (size_t)s * rdm::GRAM_BLOCK * rdm::GRAM_BLOCK;
        if (REAL) {
            re += reinterpret_cast<const double *>(slabs)[at];
        } else {
            const v2d v = reinterpret_cast<const v2d *>(slabs)[at];
            re += v.x;
            im += v.y;
        }
    }
    if (p == q) im = 0.0;
    out[p * W + q] = make_double2(re, im);
    if (p != q) out[q * W + p] = make_double2(re, -im);
}

}  // namespace ovqe
