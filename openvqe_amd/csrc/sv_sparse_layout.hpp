// sv_sparse_layout.hpp — the records, kernel arguments and dynamic-LDS layouts of the support-compacted kernels (sv_sparse.hpp), in
// plain C++: no HIP header, so that the kernels, the host sections that launch them and the host-only plan checkers
// (tests/cpu/metric_plan_check.cpp, hessian_plan_check.cpp: g++ alone) all read ONE definition of every offset.
#pragma once
#include <cstddef>
#include <cstdint>

#ifdef __HIPCC__
#define OVQE_LAYOUT_FN __host__ __device__ inline
#else
#define OVQE_LAYOUT_FN inline
#endif

namespace ovqe {

// pair word: ci (12 bits) | cj (12 bits) << 12 | sign << 24 | pattern << 25      (the metric's programs: ci is the member with the pivot
// bit clear)
struct SpOp {        // one op of a compact program: pattern p of the op -> table entry tab0 + p
    int32_t first;   // first pair
    int32_t npairs;
    int32_t tab0;    // first table entry of the op
    int32_t pad;
};
struct SpEntry {     // one entry of the Hamiltonian restricted to the support
    uint32_t ij;     // ci | cj << 12   (ci == cj: diagonal entry)
    uint32_t pad;
    double c;        // 2 * H_ij (off-diagonal, the pair counted once: ci < cj) or H_ii
};
struct DeflRow {     // one real deflation row of k_sparse_vqd_batch: [mpad] doubles at D + src * mpad, in global memory
    double beta;     // its weight
    int32_t src;
    int32_t pad;
};
struct ConRec {      // one observable of k_sparse_constrained_batch: its restricted entries [first, first + count) of the concatenated array,
    int32_t first;   // and its term linear o + quad (o - target)^2 of the cost, o = <psi|O|psi> + constant
    int32_t count;
    double constant, linear, quad, target;
};
constexpr size_t SP_CS_BYTES = 16;   // one cos/sin table entry: a double2 (sv_sparse.hpp asserts it)
static_assert(sizeof(SpOp) == 16 && sizeof(SpEntry) == 16 && sizeof(DeflRow) == 16, "16-byte records behind an even number of doubles");
static_assert(sizeof(ConRec) == 40, "five 8-byte words");

struct SparseArgs {
    int m;        // support size
    int mpad;     // per-evaluation stride of the LDS state in doubles: m rounded up to even, so that the double2 cos/sin table behind
                  // SPW states starts on a 16-byte boundary (ds_read/write_b128)
    int K;
    int nops;
    int ntab;
    int nent;
    int npairs;   // all active pairs of the program (STAGE: copied to LDS once per launch)
    int hf;       // compact slot of |hf>
    int64_t B;
    double constant;
    int dbg = 0;  // measurements ("sparse_dbg"; the rows kernels take it as a template argument): 1 no sincos, 2 no circuit rows, 3 no Hamiltonian entries, 4 (k_sparse_vqe_rows_shared) no theta loads, 5 nothing left out: wave sums by __shfl_down, as before sv_wave_reduce.hpp
};

// k_sparse_vqe
struct SpVqeLds { size_t cs, ops, pairs, bytes; };   // the spw states ([spw][mpad]) are at 0
OVQE_LAYOUT_FN SpVqeLds sp_vqe_lds(const SparseArgs &A, int spw, bool stage) {
    const size_t cs = (size_t)spw * A.mpad * sizeof(double);          // [spw][ntab], 16-byte aligned
    const size_t ops = cs + (size_t)spw * A.ntab * SP_CS_BYTES;       // [nops]   (stage)
    const size_t pairs = ops + (size_t)A.nops * sizeof(SpOp);         // [npairs] (stage)
    return {cs, ops, pairs, stage ? pairs + (size_t)A.npairs * sizeof(uint32_t) : ops};
}

// k_sparse_vqe_rows (spw = 2; mpad = support + 64 spare slots) and k_sparse_vqe_wg (spw = 1; + 128): the states, then one cos/sin
// table of ntab + 1 entries each — the last entry is the identity
struct SpRowsLds { size_t cs, bytes; };   // the states ([spw][mpad]) are at 0
OVQE_LAYOUT_FN SpRowsLds sp_rows_lds(const SparseArgs &A, int spw) {
    const size_t cs = (size_t)spw * A.mpad * sizeof(double);
    return {cs, cs + (size_t)spw * (A.ntab + 1) * SP_CS_BYTES};
}

// k_sparse_grad
struct SpGradLds { size_t lam, cs, w, gk, ops, pairs, bytes; };   // psi ([mpad]) is at 0
OVQE_LAYOUT_FN SpGradLds sp_grad_lds(const SparseArgs &A, bool stage) {
    const size_t lam = (size_t)A.mpad * sizeof(double);                  // [mpad]
    const size_t cs = 2 * lam;                                           // [ntab]
    const size_t w = cs + (size_t)A.ntab * SP_CS_BYTES;                  // [ntab]
    const size_t gk = w + (size_t)A.ntab * sizeof(double);               // [K]
    const size_t ops = gk + (size_t)((A.K + 1) & ~1) * sizeof(double);   // [nops]   (stage)
    const size_t pairs = ops + (size_t)A.nops * sizeof(SpOp);            // [npairs] (stage)
    return {lam, cs, w, gk, ops, pairs, stage ? pairs + (size_t)A.npairs * sizeof(uint32_t) : ops};
}

// k_sparse_grad_batch: nw waves per workgroup, one parameter vector per wave at a time.  Every wave has its own psi, lambda, cos/sin
// table, w and gk — the regions of sp_grad_lds at the same offsets (lam, cs, w, gk), wave v's at v * stride, the stride a multiple of
// 16 bytes; ONE copy of the op records and pair words behind the last wave serves all of them (stage)
struct SpGradBatchLds { size_t lam, cs, w, gk, stride, ops, pairs, bytes; };   // wave v's psi ([mpad]) is at v * stride
OVQE_LAYOUT_FN SpGradBatchLds sp_grad_batch_lds(const SparseArgs &A, int nw, bool stage) {
    const SpGradLds W = sp_grad_lds(A, false);
    const size_t stride = (W.bytes + 15) & ~(size_t)15;
    const size_t ops = (size_t)nw * stride;                       // [nops]   (stage)
    const size_t pairs = ops + (size_t)A.nops * sizeof(SpOp);     // [npairs] (stage)
    return {W.lam, W.cs, W.w, W.gk, stride, ops, pairs, stage ? pairs + (size_t)A.npairs * sizeof(uint32_t) : ops};
}

// k_sparse_spread_batch: k_sparse_grad_batch's arrangement with a THIRD state array per wave — psi, lambda and mu ([mpad] doubles each),
// then the cos/sin table, w and gk as in sp_grad_lds; wave v's region at v * stride, the shared op records and pair words behind the
// last wave (stage)
struct SpSpreadBatchLds { size_t lam, mu, cs, w, gk, stride, ops, pairs, bytes; };   // wave v's psi ([mpad]) is at v * stride
OVQE_LAYOUT_FN SpSpreadBatchLds sp_spread_batch_lds(const SparseArgs &A, int nw, bool stage) {
    const size_t v = (size_t)A.mpad * sizeof(double);                        // psi, lambda, mu: [mpad] each
    const size_t cs = 3 * v;                                                 // [ntab]
    const size_t w = cs + (size_t)A.ntab * SP_CS_BYTES;                      // [ntab]
    const size_t gk = w + (size_t)A.ntab * sizeof(double);                   // [K]
    const size_t region = gk + (size_t)((A.K + 1) & ~1) * sizeof(double);
    const size_t stride = (region + 15) & ~(size_t)15;
    const size_t ops = (size_t)nw * stride;                                  // [nops]   (stage)
    const size_t pairs = ops + (size_t)A.nops * sizeof(SpOp);                // [npairs] (stage)
    return {v, 2 * v, cs, w, gk, stride, ops, pairs, stage ? pairs + (size_t)A.npairs * sizeof(uint32_t) : ops};
}

// k_sparse_grad_wg
struct SpGradWgLds { size_t lam, cs, w, gk, bytes; };   // psi ([mpad] = support + 128 spare slots) is at 0
OVQE_LAYOUT_FN SpGradWgLds sp_grad_wg_lds(const SparseArgs &A) {
    const size_t lam = (size_t)A.mpad * sizeof(double);                   // [mpad]
    const size_t cs = 2 * lam;                                            // [ntab + 1]
    const size_t w = cs + (size_t)(A.ntab + 1) * SP_CS_BYTES;             // [ntab + 1], an even number of slots
    const size_t gk = w + (size_t)((A.ntab + 2) & ~1) * sizeof(double);   // [K]
    return {lam, cs, w, gk, gk + (size_t)((A.K + 1) & ~1) * sizeof(double)};
}

// k_sparse_metric
struct SpMetricArgs {
    int m, mpad, K, nops, ntab, npairs, hf;
    int64_t wpad;
};
struct SpMetricLds { size_t t, cs, dk, ops, pairs, bytes; };   // psi ([mpad]) is at 0
OVQE_LAYOUT_FN SpMetricLds sp_metric_lds(const SpMetricArgs &A, bool stage) {
    const size_t t = (size_t)A.mpad * sizeof(double);                       // [mpad]
    const size_t cs = 2 * t;                                                // [ntab]
    const size_t dk = cs + (size_t)A.ntab * SP_CS_BYTES;                    // [ntab]: coeff_e where the entry is parameter k's, else 0
    const size_t ops = dk + (size_t)((A.ntab + 1) & ~1) * sizeof(double);   // [nops]   (stage)
    const size_t pairs = ops + (size_t)A.nops * sizeof(SpOp);               // [npairs] (stage)
    return {t, cs, dk, ops, pairs, stage ? pairs + (size_t)A.npairs * sizeof(uint32_t) : ops};
}

// k_sparse_hessian
struct SpHessArgs {
    int m, mpad, K, nops, ntab, npairs, nent, hf;
    double constant;
};
struct SpHessLds { size_t t, lam, mu, cs, dk, w, wd, gk, ops, pairs, bytes; };   // psi ([mpad]) is at 0
OVQE_LAYOUT_FN SpHessLds sp_hessian_lds(const SpHessArgs &A, bool stage) {
    const size_t v = (size_t)A.mpad * sizeof(double);                                       // psi, t, lambda, mu: [mpad] each
    const size_t cs = 4 * v;                                                                // [ntab]
    const size_t dk = cs + (size_t)A.ntab * SP_CS_BYTES;                                    // [ntab]: coeff_e of parameter b's entries, else 0
    const size_t w = dk + (size_t)A.ntab * sizeof(double);                                  // [ntab]
    const size_t wd = w + (size_t)A.ntab * sizeof(double);                                  // [ntab]
    const size_t gk = wd + (size_t)A.ntab * sizeof(double);                                 // [K]
    const size_t ops = (gk + (size_t)A.K * sizeof(double) + 15) & ~(size_t)15;              // [nops]   (stage)
    const size_t pairs = ops + (size_t)A.nops * sizeof(SpOp);                               // [npairs] (stage)
    return {v, 2 * v, 3 * v, cs, dk, w, wd, gk, ops, pairs, stage ? pairs + (size_t)A.npairs * sizeof(uint32_t) : ops};
}

// the arguments of the two kernels that run the metric's compact program (metric::Compact of sv_metric_host.hpp, which takes its op
// record from this header: hence the template).  wpad / nent and constant are the caller's
template <class Compact>
SpMetricArgs sp_metric_args(const Compact &C, int K) {
    return {C.m, (C.m + 1) & ~1, K, (int)C.ops.size(), (int)C.tab.size(), (int)C.pairs.size(), C.hf, 0};
}
template <class Compact>
SpHessArgs sp_hessian_args(const Compact &C, int K, int nent, double constant) {
    return {C.m, (C.m + 1) & ~1, K, (int)C.ops.size(), (int)C.tab.size(), (int)C.pairs.size(), nent, C.hf, constant};
}

}  // namespace ovqe
