// sv_metric.hpp — streaming kernels of the Fubini-Study metric (ovqe_metric_tensor, path 2: any program on a plain handle; plan and
// store layout: sv_metric_host.hpp; launches: metric_host.inc).  The store holds 2^n rows of wpad 16-byte amplitudes, column 0 = psi,
// column 1 + k = T_k: one launch applies an op to psi and to every live tangent — the SECOND grid dimension runs over blocks of 64
// columns, a wave holds 64 consecutive columns of one row pair.  No atomics anywhere.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sv_kernels.hpp"

namespace ovqe {

enum MetricSweepKind : int32_t { MS_ROT = 0, MS_DIAG = 1, MS_X = 2, MS_H = 3, MS_CNOT = 4 };

struct MetricSweep {
    uint64_t x, z;     // MS_ROT: the string; MS_DIAG: z; MS_X / MS_H / MS_CNOT: x = the (target) bit
    int32_t kind;
    int32_t pivot;     // highest bit of x
    int32_t ctrl;      // MS_CNOT: control bit
    int32_t ny;        // popcount(x & z) & 3
    double c, s;       // cos / sin of the angle
};

// -i i^ny v: the factor of exp(-i phi P) = cos(phi) - i sin(phi) P in front of the permuted amplitude
__device__ inline v2d metric_mulf(v2d v, int ny) {
    switch (ny & 3) {
    case 0: return v2d{v.y, -v.x};
    case 1: return v;
    case 2: return v2d{-v.y, v.x};
    default: return v2d{-v.x, -v.y};
    }
}

__global__ __launch_bounds__(64) void k_metric_seed(v2d *__restrict__ V, uint64_t hf, int64_t wpad) {
    if (blockIdx.x == 0 && threadIdx.x == 0) V[hf * (uint64_t)wpad] = v2d{1.0, 0.0};
}

// block = 4 rows (pairs) x 64 columns; grid.x strides over the nwork row pairs (MS_DIAG: rows), grid.y over the live column blocks
__global__ __launch_bounds__(256) void k_metric_sweep(v2d *__restrict__ V, uint64_t nwork, int64_t wpad, int ncols, MetricSweep S) {
    const int col = (int)blockIdx.y * 64 + (int)(threadIdx.x & 63);
    if (col >= ncols) return;
    const uint64_t low = (1ull << S.pivot) - 1ull;
    for (uint64_t p = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6); p < nwork; p += (uint64_t)gridDim.x * 4u) {
        if (S.kind == MS_DIAG) {   // a (c - i s sigma), sigma = (-1)^{parity(i & z)}
            v2d *a = V + p * (uint64_t)wpad + col;
            const double sg = (__builtin_popcountll(p & S.z) & 1) ? -S.s : S.s;
            const v2d v = *a;
            *a = v2d{v.x * S.c + v.y * sg, v.y * S.c - v.x * sg};
            continue;
        }
        const uint64_t i0 = ((p & ~low) << 1) | (p & low), j = i0 ^ S.x;
        v2d *pu = V + i0 * (uint64_t)wpad + col, *pv = V + j * (uint64_t)wpad + col;
        const v2d u = *pu, v = *pv;
        if (S.kind == MS_ROT) {   // a'_i = c a_i + s (-i i^ny) (-1)^{parity((i ^ x) & z)} a_{i ^ x}
            const double si = (__builtin_popcountll(j & S.z) & 1) ? -S.s : S.s;
            const double sj = (__builtin_popcountll(i0 & S.z) & 1) ? -S.s : S.s;
            const v2d fv = metric_mulf(v, S.ny), fu = metric_mulf(u, S.ny);
            *pu = v2d{S.c * u.x + si * fv.x, S.c * u.y + si * fv.y};
            *pv = v2d{S.c * v.x + sj * fu.x, S.c * v.y + sj * fu.y};
        } else if (S.kind == MS_X) {
            *pu = v;
            *pv = u;
        } else if (S.kind == MS_H) {
            const double r = 0.70710678118654752440;
            *pu = v2d{r * (u.x + v.x), r * (u.y + v.y)};
            *pv = v2d{r * (u.x - v.x), r * (u.y - v.y)};
        } else if ((i0 >> S.ctrl) & 1ull) {   // MS_CNOT
            *pu = v;
            *pv = u;
        }
    }
}

// T_k += coeff (-i P) psi on the state AFTER the rotation: column `col` += coeff (-i i^ny) (-1)^{parity((i ^ x) & z)} psi_{i ^ x}
__global__ __launch_bounds__(256) void k_metric_add(v2d *__restrict__ V, uint64_t nrows, int64_t wpad, int col, uint64_t x, uint64_t z, int ny,
                                                    double coeff) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < nrows; i += (uint64_t)gridDim.x * 256u) {
        const uint64_t j = i ^ x;
        const v2d f = metric_mulf(V[j * (uint64_t)wpad], ny);
        const double sg = (__builtin_popcountll(j & z) & 1) ? -coeff : coeff;
        v2d *t = V + i * (uint64_t)wpad + col;
        const v2d a = *t;
        *t = v2d{a.x + sg * f.x, a.y + sg * f.y};
    }
}

}  // namespace ovqe
