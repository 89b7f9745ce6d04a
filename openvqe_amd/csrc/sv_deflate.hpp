// sv_deflate.hpp — kernels of the deflated energies and gradients (ovqe_deflated_gradient_batch; host section: deflate_host.inc; the
// compact kernel itself, k_sparse_vqd_batch, sits next to k_sparse_grad_batch in sv_sparse.hpp).
//
//   k_deflate_gather   compact path: the stored vectors restricted to the compact support, as real rows D[2 j] = Re phi_j,
//                      D[2 j + 1] = Im phi_j over the slots of the compact state
//   k_deflate_dots     streaming path: up to four overlaps <phi_j|psi> per pass over psi, one partial per workgroup and vector
//   k_deflate_axpy     streaming path: lambda += sum_j beta_j o_j phi_j, up to four vectors per pass, o_j read from the device
// All accesses to the register are one 16-byte amplitude per lane, consecutive lanes on consecutive amplitudes.
#pragma once

#include "sv_kernels.hpp"

namespace ovqe {

constexpr int DEFLATE_MAX = 32;     // vectors a handle holds
constexpr int DEFLATE_CHUNK = 4;    // vectors per pass of the streaming kernels

struct DeflVecs { const amp_t *v[DEFLATE_MAX]; };
struct DeflChunk {
    const amp_t *v[DEFLATE_CHUNK];
    double beta[DEFLATE_CHUNK];
    int count;
};

// D[(2 j + c) * mpad + i] = (c ? Im : Re) phi_j[basis[i]]; slots without a basis state (basis[i] >= namps: the padding) give 0.
// im_flag[j] becomes 1 when Im phi_j is non-zero somewhere on the support (every writer stores the same value).  Grid (slots / 256, J).
__global__ __launch_bounds__(256) void k_deflate_gather(DeflVecs V, const uint64_t *__restrict__ basis, int mpad, uint64_t namps,
                                                        double *__restrict__ D, int *__restrict__ im_flag) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x), j = (int)blockIdx.y;
    if (i >= mpad) return;
    const uint64_t a = basis[i];
    const amp_t v = a < namps ? V.v[j][a] : make_double2(0.0, 0.0);
    D[(size_t)(2 * j) * mpad + i] = v.x;
    D[(size_t)(2 * j + 1) * mpad + i] = v.y;
    if (v.y != 0.0) im_flag[j] = 1;
}

// partials[k * gridDim.x + block] = sum over the block's grid-stride slice of conj(phi_k[i]) psi[i], k < C.count: the order inside a
// block is block_sum's, the blocks are summed by k_reduce — the same bits from call to call
__global__ __launch_bounds__(256) void k_deflate_dots(DeflChunk C, const amp_t *__restrict__ psi, uint64_t namps,
                                                      double2 *__restrict__ partials) {
    __shared__ double2 red[4];
    double2 acc[DEFLATE_CHUNK];
#pragma unroll
    for (int k = 0; k < DEFLATE_CHUNK; ++k) acc[k] = make_double2(0.0, 0.0);
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < namps; i += stride) {
        const amp_t p = psi[i];
#pragma unroll
        for (int k = 0; k < DEFLATE_CHUNK; ++k)
            if (k < C.count) {
                const amp_t f = C.v[k][i];
                acc[k].x += f.x * p.x + f.y * p.y;
                acc[k].y += f.x * p.y - f.y * p.x;
            }
    }
#pragma unroll
    for (int k = 0; k < DEFLATE_CHUNK; ++k)
        if (k < C.count) {
            const double2 t = block_sum<256>(acc[k], red);
            if (threadIdx.x == 0) partials[(size_t)k * gridDim.x + blockIdx.x] = t;
        }
}

// lam[i] += sum_{k < C.count} C.beta[k] o[k] C.v[k][i]   (o: complex, on the device)
__global__ __launch_bounds__(256) void k_deflate_axpy(DeflChunk C, const double2 *__restrict__ o, amp_t *__restrict__ lam, uint64_t namps) {
    double2 c[DEFLATE_CHUNK];
#pragma unroll
    for (int k = 0; k < DEFLATE_CHUNK; ++k) {
        const double2 ok = k < C.count ? o[k] : make_double2(0.0, 0.0);
        c[k] = make_double2(C.beta[k] * ok.x, C.beta[k] * ok.y);
    }
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < namps; i += stride) {
        amp_t r = lam[i];
#pragma unroll
        for (int k = 0; k < DEFLATE_CHUNK; ++k)
            if (k < C.count) {
                const amp_t f = C.v[k][i];
                r.x += c[k].x * f.x - c[k].y * f.y;
                r.y += c[k].x * f.y + c[k].y * f.x;
            }
        lam[i] = r;
    }
}

}  // namespace ovqe
