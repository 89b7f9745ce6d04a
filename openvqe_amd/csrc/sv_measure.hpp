// sv_measure.hpp — kernels of finite-shot measurement (plan and geometry: sv_measure_host.hpp; launches: measure_host.inc).
//
//   k_meas_tile          phi = B psi for the rotated bits inside an LDS tile of 2^tile_bits amplitudes, fused with the copy out of the
//                        state buffer (which is only read); writes phi when passes above the tile follow, else p = |phi|^2
//   k_meas_high          one rotated bit above the tile, in place on phi; the last such pass writes p
//   k_meas_scan_chunks   inclusive scan of p inside chunks of SCAN_CHUNK elements, in place, + the chunk totals
//   k_meas_scan_totals   inclusive scan of the chunk totals by one workgroup (256 at a time with a carry: one stage at every size)
//   k_meas_scan_offsets  chunk b > 0 takes the total in front of it
//   k_meas_draw          one lane per shot: uniform, binary search of u W in the prefix array, step off zero-probability indices,
//                        signs of the group's terms; per term one ballot + popcount and one integer atomic per wave; (v, v^2) per wave
//   k_meas_finish        the per-wave partials added as a fixed balanced tree
//
// THE PREFIX ARRAY.  C_i = sum_{j <= i} p_j with a fixed association (thread runs of 8, a shuffle scan per wave, the waves and chunks in
// order), so a call gives the same bits every time; the array is monotone only up to rounding where runs, waves and chunks meet.  The
// SIGN BIT of entry i is set iff p_i == 0 (p and C are never negative, and -0.0 carries the mark for a zero prefix): the draw reads
// magnitudes, and an outcome that lands on a marked index moves to the next unmarked one (the previous one when none follows), which
// shares its exact prefix value — so an index of probability zero is never returned, whatever the rounding of the scan did.  W is the
// magnitude of the last entry.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sv_kernels.hpp"
#include "sv_measure_host.hpp"

namespace ovqe {

// (a0, a1) on one rotated bit: H, or H S^+ (y): a1 takes -i first
__device__ __forceinline__ void meas_butterfly(double2 &a0, double2 &a1, bool y) {
    constexpr double R = 0.70710678118654752440;
    const double2 w = y ? make_double2(a1.y, -a1.x) : a1;
    const double2 s = make_double2((a0.x + w.x) * R, (a0.y + w.y) * R);
    const double2 d = make_double2((a0.x - w.x) * R, (a0.y - w.y) * R);
    a0 = s;
    a1 = d;
}

// grid: 2^(n - tile_bits) workgroups of 256 threads; dynamic LDS: 16 B << tile_bits when a bit is rotated
__global__ __launch_bounds__(256) void k_meas_tile(const amp_t *__restrict__ psi, int tile_bits, uint64_t low_x, uint64_t low_y,
                                                   amp_t *__restrict__ phi, double *__restrict__ p) {
    extern __shared__ double2 meas_tile[];
    const uint32_t TS = 1u << tile_bits;
    const uint64_t base = (uint64_t)blockIdx.x << tile_bits;
    const uint64_t low = low_x | low_y;
    if (low == 0) {   // nothing to rotate in the tile: no LDS round trip
        for (uint32_t k = threadIdx.x; k < TS; k += 256) {
            const amp_t a = psi[base + k];
            if (phi) phi[base + k] = a;
            if (p) p[base + k] = a.x * a.x + a.y * a.y;
        }
        return;
    }
    for (uint32_t k = threadIdx.x; k < TS; k += 256) meas_tile[k] = psi[base + k];
    for (int b = 0; b < tile_bits; ++b) {
        if (!((low >> b) & 1ull)) continue;
        const bool y = (low_y >> b) & 1ull;
        __syncthreads();
        for (uint32_t k = threadIdx.x; k < (TS >> 1); k += 256) {
            const uint32_t i0 = ((k >> b) << (b + 1)) | (k & ((1u << b) - 1u)), i1 = i0 | (1u << b);
            double2 a0 = meas_tile[i0], a1 = meas_tile[i1];
            meas_butterfly(a0, a1, y);
            meas_tile[i0] = a0;
            meas_tile[i1] = a1;
        }
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < TS; k += 256) {
        const double2 a = meas_tile[k];
        if (phi) phi[base + k] = a;
        if (p) p[base + k] = a.x * a.x + a.y * a.y;
    }
}

// grid-stride over the 2^(n-1) pairs of bit `bit`
__global__ __launch_bounds__(256) void k_meas_high(amp_t *__restrict__ phi, uint64_t npairs, int bit, int y, double *__restrict__ p) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x; k < npairs; k += stride) {
        const uint64_t i0 = ((k >> bit) << (bit + 1)) | (k & ((1ull << bit) - 1ull)), i1 = i0 | (1ull << bit);
        double2 a0 = phi[i0], a1 = phi[i1];
        meas_butterfly(a0, a1, y != 0);
        phi[i0] = a0;
        phi[i1] = a1;
        if (p) {
            p[i0] = a0.x * a0.x + a0.y * a0.y;
            p[i1] = a1.x * a1.x + a1.y * a1.y;
        }
    }
}

// scan of one value per thread over a workgroup of 256 (every thread active): -> the inclusive sum, *excl the exclusive one.  Fixed
// association: Hillis-Steele inside a wave, the waves' totals in order.
__device__ __forceinline__ double meas_block_scan(double v, double *wave_tot, double *excl) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    double inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double o = __shfl_up(inc, off);
        if (lane >= off) inc += o;
    }
    const double before = __shfl_up(inc, 1);
    if (lane == 63) wave_tot[w] = inc;
    __syncthreads();
    double base = 0.0;
    for (int k = 0; k < w; ++k) base += wave_tot[k];
    __syncthreads();   // (wave_tot is free again)
    *excl = lane ? base + before : base;
    return base + inc;
}

// grid: one workgroup per chunk.  In: p.  Out: the chunk-local inclusive sums, sign bit set where p == 0; totals[chunk] = the last one
__global__ __launch_bounds__(measure::SCAN_THREADS) void k_meas_scan_chunks(double *__restrict__ C, uint64_t N, double *__restrict__ totals) {
    __shared__ double wave_tot[4];
    constexpr int U = measure::SCAN_PER_THREAD;
    const uint64_t i0 = (uint64_t)blockIdx.x * measure::SCAN_CHUNK + (uint64_t)threadIdx.x * U;
    double p[U], r[U];
    if (i0 + U <= N) {
        const double2 *src = (const double2 *)(C + i0);
#pragma unroll
        for (int k = 0; k < U / 2; ++k) {
            const double2 t = src[k];
            p[2 * k] = t.x;
            p[2 * k + 1] = t.y;
        }
    } else {
#pragma unroll
        for (int k = 0; k < U; ++k) p[k] = i0 + k < N ? C[i0 + k] : 0.0;
    }
    double run = 0.0;
#pragma unroll
    for (int k = 0; k < U; ++k) {
        run += p[k];
        r[k] = run;
    }
    double off;
    (void)meas_block_scan(run, wave_tot, &off);
#pragma unroll
    for (int k = 0; k < U; ++k) {
        const double c = off + r[k];
        if (i0 + k < N) C[i0 + k] = p[k] > 0.0 ? c : -c;
    }
    if (threadIdx.x == measure::SCAN_THREADS - 1) totals[blockIdx.x] = off + r[U - 1];
}

// one workgroup: totals -> their inclusive sums, 256 at a time, the carry = what the last thread of the step before wrote
__global__ __launch_bounds__(256) void k_meas_scan_totals(double *__restrict__ totals, uint64_t chunks) {
    __shared__ double wave_tot[4];
    __shared__ double carry_s;
    double carry = 0.0;
    for (uint64_t b0 = 0; b0 < chunks; b0 += 256) {
        const uint64_t i = b0 + threadIdx.x;
        double excl;
        const double out = carry + meas_block_scan(i < chunks ? totals[i] : 0.0, wave_tot, &excl);
        if (i < chunks) totals[i] = out;
        if (threadIdx.x == 255) carry_s = out;
        __syncthreads();
        carry = carry_s;
        __syncthreads();
    }
}

// grid: chunks - 1 workgroups; chunk b = blockIdx.x + 1 takes totals[b - 1]
__global__ __launch_bounds__(measure::SCAN_THREADS) void k_meas_scan_offsets(double *__restrict__ C, uint64_t N, const double *__restrict__ totals) {
    constexpr int U = measure::SCAN_PER_THREAD;
    const uint64_t b = (uint64_t)blockIdx.x + 1;
    const double off = totals[b - 1];
    const uint64_t i0 = b * measure::SCAN_CHUNK + (uint64_t)threadIdx.x * U;
#pragma unroll
    for (int k = 0; k < U; ++k)
        if (i0 + k < N) {
            const double c = C[i0 + k];
            C[i0 + k] = copysign(fabs(c) + off, c);
        }
}

__device__ __forceinline__ bool meas_marked(double c) { return __double2hiint(c) < 0; }

// one lane per shot; grid: ceil(n_shots / 256).  partials[global wave] = (sum v, sum v^2) of the wave's shots.  term_sums (may be
// null) must be zero on entry.  Nothing is drawn when W is not a positive finite number (the host reports it).
__global__ __launch_bounds__(measure::DRAW_THREADS) void k_meas_draw(const double *__restrict__ C, uint64_t N, int64_t n_shots, uint64_t key,
                                                                     uint64_t first_shot, int T, const uint64_t *__restrict__ mask,
                                                                     const double *__restrict__ coeff,
                                                                     unsigned long long *__restrict__ term_sums,
                                                                     double2 *__restrict__ partials, uint64_t *__restrict__ indices) {
    const int64_t gid = (int64_t)blockIdx.x * measure::DRAW_THREADS + threadIdx.x;
    const bool active = gid < n_shots;
    const double W = fabs(C[N - 1]);
    uint64_t b = 0;
    if (active && W > 0.0 && W <= 1.79769313486231570815e308) {
        const uint64_t s = first_shot + (uint64_t)gid;
        const double u = (double)(mix64(key ^ mix64(s)) >> 11) * (1.0 / 9007199254740992.0);
        const double t = u * W;
        uint64_t lo = 0, hi = N;   // the smallest i with |C_i| > t
        while (lo < hi) {
            const uint64_t mid = lo + ((hi - lo) >> 1);
            if (fabs(C[mid]) > t) hi = mid;
            else lo = mid + 1;
        }
        b = lo < N ? lo : N - 1;
        if (meas_marked(C[b])) {   // p_b == 0: the next index with p > 0, the previous one when the rest is zero
            uint64_t j = b + 1;
            while (j < N && meas_marked(C[j])) ++j;
            if (j >= N) {
                j = b;
                while (j > 0 && meas_marked(C[j])) --j;
            }
            b = j;
        }
        if (indices) indices[gid] = b;
    }
    const int act = __popcll(__ballot(active));   // (the tail wave's idle lanes are not counted)
    const int lane = threadIdx.x & 63;
    double v = 0.0;
    for (int t = 0; t < T; ++t) {
        const uint64_t m = mask[t];
        const double c = coeff[t];
        const bool one = active && (__popcll(b & m) & 1);
        const int ones = __popcll(__ballot(one));
        if (term_sums && lane == 0) atomicAdd(&term_sums[t], (unsigned long long)(long long)(act - 2 * ones));
        v += one ? -c : c;
    }
    if (!active) v = 0.0;
    double v2 = v * v;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        v += __shfl_xor(v, off);
        v2 += __shfl_xor(v2, off);
    }
    if (lane == 0) partials[gid >> 6] = make_double2(v, v2);
}

// one workgroup: partials[0] = the sum of the P partials as a balanced tree over L = the power of two >= P (element i meets
// element i + L/2, then i + L/4, ...; equal addends of a power-of-two count add without rounding), -> out = (sum v, sum v^2, W)
__global__ __launch_bounds__(256) void k_meas_finish(double2 *partials, int64_t P, int64_t L, const double *C, uint64_t N, double *out) {
    for (int64_t len = L >> 1; len >= 1; len >>= 1) {
        for (int64_t i = threadIdx.x; i < len; i += 256)
            if (i + len < P) {
                const double2 a = partials[i], c = partials[i + len];
                partials[i] = make_double2(a.x + c.x, a.y + c.y);
            }
        __threadfence_block();
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[0] = P > 0 ? partials[0].x : 0.0;
        out[1] = P > 0 ? partials[0].y : 0.0;
        out[2] = fabs(C[N - 1]);
    }
}

}  // namespace ovqe
