// sv_subspace.hpp — kernels of the subspace-expansion matrices S_ij = <phi_i|phi_j>, G_ij = <phi_i|H|phi_j>, phi_j = O_j psi (plan and
// index arithmetic: sv_subspace_host.hpp; launches: subspace_host.inc).  The state buffer is only read.  No atomics: every partial sum
// has one owner and the slabs are reduced in slice order, so a call gives the same bits every time.
//   k_sub_shadow       bitmap of the rows R: the support bitmap of psi (k_rdm_census) moved by every distinct x mask of the pool, ORed
//   k_sub_expand       Phi[row][j] = (O_j psi)[index(row)] into the index-major store, psi gathered straight from the state buffer
//   k_sub_sigma        Sigma[row][0..m) = constant Phi[row] + sum_g D_g Phi[pos(index(row) ^ x_g)]: D_g once per row, lanes over columns
//   k_sub_gram         partial Gram blocks conj(A)^T B per (block pair, row slice): the S pairs and the Phi^H Sigma pairs in one launch
//   k_sub_finish_full  sum of the slabs of Phi^H Sigma in slice order, all m x m entries as computed (S goes through k_rdm_finish)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sv_kernels.hpp"
#include "sv_rdm.hpp"
#include "sv_subspace_host.hpp"

namespace ovqe {

__global__ __launch_bounds__(256) void k_sub_shadow(const uint64_t *__restrict__ in, uint64_t *__restrict__ out, uint64_t nwords,
                                                    const uint64_t *__restrict__ xs, int nx) {
    const uint64_t w = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (w >= nwords) return;
    uint64_t v = 0;
    for (int k = 0; k < nx; ++k) v |= sub::xor_word(in, w, xs[k]);
    out[w] = v;
}

// element e of the store's Phi half is (row e / mb, column e % mb); mb is a multiple of 64, so a wave holds 64 consecutive columns of
// ONE row and its stores are one contiguous run.  Columns from m on are zero.  Operator j is the terms [off[j], off[j + 1]) in the
// caller's order, i^ny folded into the coefficient; term t contributes c_t (-1)^{popcount(k & z_t)} psi[k], k = index ^ x_t.
template <bool DENSE>
__global__ __launch_bounds__(256) void k_sub_expand(const amp_t *__restrict__ st, const uint64_t *__restrict__ rows, int64_t nrows,
                                                    const int64_t *__restrict__ off, const uint64_t *__restrict__ xs,
                                                    const HTerm *__restrict__ terms, int64_t m, int64_t mb, int64_t wpad,
                                                    v2d *__restrict__ store) {
    const uint64_t total = (uint64_t)nrows * (uint64_t)mb;
    for (uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x; e < total; e += (uint64_t)gridDim.x * 256u) {
        const uint64_t r = e / (uint64_t)mb;
        const int64_t c = (int64_t)(e - r * (uint64_t)mb);
        double sx = 0.0, sy = 0.0;
        if (c < m) {
            const uint64_t i = DENSE ? r : rows[r];
            for (int64_t t = off[c]; t < off[c + 1]; ++t) {
                const uint64_t k = i ^ xs[t];
                const HTerm ht = terms[t];
                const amp_t a = st[k];
                const double sg = parity_sign64(k & ht.z);
                const double dr = ht.cr * sg, di = ht.ci * sg;
                sx += dr * a.x - di * a.y;
                sy += dr * a.y + di * a.x;
            }
        }
        store[r * (uint64_t)wpad + (uint64_t)c] = v2d{sx, sy};
    }
}

__device__ __forceinline__ double sub_lane_double(double v, int lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ uint64_t sub_lane_u64(uint64_t v, int lane) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
    return ((uint64_t)hi << 32) | lo;
}

// One wave per row, sub::SIGMA_ROW_TILE rows per workgroup; blockIdx.y picks NB column blocks of 64 (lane = column inside a block).
// Per batch of sub::SIGMA_GROUP_BATCH x-groups, lane l computes the coefficient of group g0 + l on this row — D_g(k) = sum_t c_t
// (-1)^{popcount(k & z_t)} on the partner k = index ^ x_g, the sum and the snap of k_apply_sum — and the partner's position in the
// store; a partner outside R holds exact zeros in every column and is dropped with the groups whose coefficient is zero.  The
// surviving (coefficient, position) pairs are handed round the wave in group order and every lane adds D * Phi[partner][column] to
// its NB accumulators: T sign evaluations per row instead of T per row and column, one contiguous read of 1 KiB per partner and block.
template <bool DENSE, int NB>
__global__ __launch_bounds__(sub::SIGMA_THREADS) void k_sub_sigma(v2d *__restrict__ store, const uint64_t *__restrict__ rows, int64_t nrows,
                                                                  const uint64_t *__restrict__ bitmap, const uint64_t *__restrict__ start,
                                                                  const HGroup *__restrict__ groups, int ngroups,
                                                                  const HTerm *__restrict__ terms, double constant, int nb, int64_t mb,
                                                                  int64_t wpad) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int blk0 = blockIdx.y * NB;
    for (int64_t r = (int64_t)blockIdx.x * sub::SIGMA_ROW_TILE + wave; r < nrows; r += (int64_t)gridDim.x * sub::SIGMA_ROW_TILE) {
        const uint64_t i = DENSE ? (uint64_t)r : rows[r];
        v2d acc[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            acc[b] = v2d{0.0, 0.0};
            if (blk0 + b < nb) acc[b] = constant * store[(uint64_t)r * (uint64_t)wpad + (uint64_t)(blk0 + b) * 64u + lane];
        }
        for (int g0 = 0; g0 < ngroups; g0 += sub::SIGMA_GROUP_BATCH) {
            double dr = 0.0, di = 0.0;
            uint64_t pos = 0;
            bool live = false;
            if (g0 + lane < ngroups) {
                const HGroup gr = groups[g0 + lane];
                const uint64_t k = i ^ gr.x;
                if (DENSE || sub::in_rows(bitmap, k)) {
                    for (int t = gr.t0; t < gr.t1; ++t) {
                        const HTerm ht = terms[t];
                        const double sg = parity_sign64(k & ht.z);
                        dr = fma(ht.cr, sg, dr);
                        di = fma(ht.ci, sg, di);
                    }
                    group_coeff_snap(dr, di, gr.tiny);
                    live = dr != 0.0 || di != 0.0;
                    pos = DENSE ? k : sub::row_position(bitmap, start, k);
                }
            }
            uint64_t todo = __ballot(live);
            while (todo) {
                const int l = __builtin_ctzll(todo);
                todo &= todo - 1;
                const double cr = sub_lane_double(dr, l), ci = sub_lane_double(di, l);
                const v2d *src = store + sub_lane_u64(pos, l) * (uint64_t)wpad + lane;
#pragma unroll
                for (int b = 0; b < NB; ++b)
                    if (blk0 + b < nb) {
                        const v2d a = src[(uint64_t)(blk0 + b) * 64u];
                        acc[b].x = fma(-ci, a.y, fma(cr, a.x, acc[b].x));
                        acc[b].y = fma(ci, a.x, fma(cr, a.y, acc[b].y));
                    }
            }
        }
#pragma unroll
        for (int b = 0; b < NB; ++b)
            if (blk0 + b < nb) store[(uint64_t)r * (uint64_t)wpad + (uint64_t)mb + (uint64_t)(blk0 + b) * 64u + lane] = acc[b];
    }
}

// Workgroup blockIdx.x = pair * slices + slice: slab[p][q] = sum over the slice's rows of conj(V[row][I * 64 + p]) V[row][J * 64 + q],
// (I, J) from sub::block_pair.  The arithmetic and the thread tile of k_rdm_gram's 16-byte form; a slice without rows stores zeros.
__global__ __launch_bounds__(rdm::GRAM_THREADS) void k_sub_gram(const v2d *__restrict__ V, int64_t nrows, int64_t wpad, int nb, int slices,
                                                                int64_t slice_rows, v2d *__restrict__ slabs) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int TR = sub::GRAM_TILE_ROWS;
    constexpr int UPR = rdm::GRAM_BLOCK;                                   // 16-byte units of one row of a block
    constexpr int UNITS = rdm::GRAM_TILE_BYTES / 16 / rdm::GRAM_THREADS;   // units a thread stages per tile
    constexpr sub::GramLds L = sub::gram_lds();
    v2d *la = reinterpret_cast<v2d *>(smem);
    v2d *lb = reinterpret_cast<v2d *>(smem + L.b);
    const int pair = blockIdx.x / slices, slice = blockIdx.x - pair * slices;
    const int64_t r_begin = (int64_t)slice * slice_rows;
    const int64_t r_end = r_begin + slice_rows < nrows ? r_begin + slice_rows : nrows;
    int I, J;
    sub::block_pair(pair, nb, &I, &J);
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
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
                const v2d *src = V + (uint64_t)(r0 + row) * (uint64_t)wpad;
                ga[u] = src[(uint64_t)I * rdm::GRAM_BLOCK + cu];
                gb[u] = src[(uint64_t)J * rdm::GRAM_BLOCK + cu];
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
    const size_t slab = (size_t)blockIdx.x * rdm::GRAM_BLOCK * rdm::GRAM_BLOCK;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            slabs[slab + (size_t)rdm::owned_column(false, ty, i) * rdm::GRAM_BLOCK + rdm::owned_column(false, tx, j)] = v2d{acc_re[i][j], acc_im[i][j]};
}

// out[p][q] (m x m complex, row-major) = <phi_p|sigma_q> from the slabs of pair sub::h_pair_index(p / 64, q / 64) summed in slice
// order: every entry as computed, no mirror
__global__ __launch_bounds__(256) void k_sub_finish_full(const v2d *__restrict__ slabs, int64_t m, int nb, int slices, double2 *__restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= m * m) return;
    const int64_t p = e / m, q = e - p * m;
    const int I = (int)(p / rdm::GRAM_BLOCK), J = (int)(q / rdm::GRAM_BLOCK);
    const size_t first = (size_t)sub::h_pair_index(I, J, nb) * slices * rdm::GRAM_BLOCK * rdm::GRAM_BLOCK +
                         (size_t)(p - (int64_t)I * rdm::GRAM_BLOCK) * rdm::GRAM_BLOCK + (size_t)(q - (int64_t)J * rdm::GRAM_BLOCK);
    double re = 0.0, im = 0.0;
    for (int s = 0; s < slices; ++s) {
        const v2d v = slabs[first + (size_t)s * rdm::GRAM_BLOCK * rdm::GRAM_BLOCK];
        re += v.x;
        im += v.y;
    }
    out[e] = make_double2(re, im);
}

}  // namespace ovqe
