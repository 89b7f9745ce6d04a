// sv_hessian.hpp — streaming kernels of the exact energy Hessian (ovqe_energy_hessian, path 2: any program on a plain handle; the
// derivation: sv_hessian_host.hpp; launches: hessian_host.inc; path 1 is k_sparse_hessian in sv_sparse.hpp).  Two index-major stores in
// the metric's layout (sv_metric.hpp): A holds psi in column 0 and T_k = d psi / d theta_k in column 1 + k, Sigma = H A column by column.
// The op list is walked backwards with k_metric_sweep on both stores; at a parameterised rotation k_hess_weights reads
//   val_c = Im( <Sigma_c|P|A_0> + <Sigma_0|P|A_c> )        c = 0: the gradient's w_r;  c = 1 + b: w'_r / 2 of the direction b
// for all columns at once, and k_metric_add (with -coeff) injects coeff (i P) of column 0 into column 1 + pidx of both stores.  Sums are
// taken in a fixed order — a thread's rows, the four row lanes of a workgroup, the slabs — and nothing is added atomically: the result
// is bit-identical from call to call.  O(K R) sweeps of the register for R rotations: meant for small registers and short programs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sv_cover_host.hpp"
#include "sv_metric.hpp"

namespace ovqe {

// i^ny v
__device__ inline v2d hess_iny(v2d v, int ny) {
    switch (ny & 3) {
    case 0: return v;
    case 1: return v2d{-v.y, v.x};
    case 2: return v2d{-v.x, -v.y};
    default: return v2d{v.y, -v.x};
    }
}

// one x-group of the Hamiltonian on every column: Sigma[i, col] += sum_t (cr_t + i ci_t) (-1)^{parity((i ^ x) & z_t)} A[i ^ x, col]
// (i^ny is folded into cr + i ci).  block = 4 rows x 64 columns, as k_metric_sweep; a thread owns its (row, column) slots: no atomics
__global__ __launch_bounds__(256) void k_hess_apply(const v2d *__restrict__ A, v2d *__restrict__ S, uint64_t nrows, int64_t wpad, int ncols,
                                                    uint64_t x, const HTerm *__restrict__ terms, int t0, int t1) {
    const int col = (int)blockIdx.y * 64 + (int)(threadIdx.x & 63);
    if (col >= ncols) return;
    for (uint64_t i = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6); i < nrows; i += (uint64_t)gridDim.x * 4u) {
        const uint64_t j = i ^ x;
        double dr = 0.0, di = 0.0;
        for (int t = t0; t < t1; ++t) {
            const HTerm ht = terms[t];
            const bool neg = (__builtin_popcountll(j & ht.z) & 1) != 0;
            dr += neg ? -ht.cr : ht.cr;
            di += neg ? -ht.ci : ht.ci;
        }
        const v2d v = A[j * (uint64_t)wpad + col];
        v2d *s = S + i * (uint64_t)wpad + col;
        const v2d a = *s;
        *s = v2d{a.x + dr * v.x - di * v.y, a.y + dr * v.y + di * v.x};
    }
}

// partial[slab, col] = sum over the slab's rows of val_col (above) with (P a)_i = i^ny (-1)^{parity((i ^ x) & z)} a_{i ^ x};
// energy != 0: of Re conj(A[i, col]) Sigma[i, 0] instead (column 0: <psi|H|psi>).  grid = (slabs, column blocks), block = 4 rows x 64 columns
__global__ __launch_bounds__(256) void k_hess_weights(const v2d *__restrict__ A, const v2d *__restrict__ S, uint64_t nrows, uint64_t slab_rows,
                                                      int64_t wpad, int ncols, uint64_t x, uint64_t z, int ny, int energy,
                                                      double *__restrict__ partial) {
    __shared__ double red[256];
    const int tid = (int)threadIdx.x, col = (int)blockIdx.y * 64 + (tid & 63);
    const uint64_t r0 = (uint64_t)blockIdx.x * slab_rows, r1 = r0 + slab_rows < nrows ? r0 + slab_rows : nrows;
    double acc = 0.0;
    if (col < ncols)
        for (uint64_t i = r0 + (uint64_t)(tid >> 6); i < r1; i += 4u) {
            const v2d s0 = S[i * (uint64_t)wpad];
            if (energy) {
                const v2d a = A[i * (uint64_t)wpad + col];
                acc += a.x * s0.x + a.y * s0.y;
                continue;
            }
            const uint64_t j = i ^ x;
            const v2d p0 = hess_iny(A[j * (uint64_t)wpad], ny), pc = hess_iny(A[j * (uint64_t)wpad + col], ny);
            const v2d sc = S[i * (uint64_t)wpad + col];
            const double v = (sc.x * p0.y - sc.y * p0.x) + (s0.x * pc.y - s0.y * pc.x);   // Im(conj(s) p) = s.x p.y - s.y p.x
            acc += (__builtin_popcountll(j & z) & 1) ? -v : v;
        }
    red[tid] = acc;
    __syncthreads();
    if (tid < 64 && col < ncols) partial[(uint64_t)blockIdx.x * (uint64_t)wpad + col] = ((red[tid] + red[tid + 64]) + red[tid + 128]) + red[tid + 192];
}

// out[col] = the slabs of a column summed in slab order
__global__ __launch_bounds__(64) void k_hess_weights_finish(const double *__restrict__ partial, int nslabs, int64_t wpad, int ncols,
                                                            double *__restrict__ out) {
    const int col = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (col >= ncols) return;
    double acc = 0.0;
    for (int s = 0; s < nslabs; ++s) acc += partial[(uint64_t)s * (uint64_t)wpad + col];
    out[col] = acc;
}

}  // namespace ovqe
