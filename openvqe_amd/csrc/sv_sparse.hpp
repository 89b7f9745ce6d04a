// sv_sparse.hpp — support-compacted evaluation: E(theta) on the REACHABLE SUPPORT of the circuit.
//
// A fused OP_TAB pass (sv_small.hpp) never touches a pair whose rotation angle is structurally zero, so an
// amplitude that is not reachable from |HF> through the active pairs of the program is exactly 0.0 for every
// parameter vector.  The host propagates that support through the program once (ovqe_sv.hip,
// build_sparse_program): S_0 = {hf}, S_k = S_{k-1} + partners of S_{k-1} under the active pairs of op k.  For a
// particle-number / spin conserving ansatz on a Hartree-Fock determinant this is the CI space of the sector
// (H2O/STO-3G: 441 of 16384 amplitudes); nothing about fermions is assumed — the analysis is on Pauli masks.
//
// When the support is small the whole evaluation is re-expressed on compact indices 0..m-1:
//   * per op: the list of active pairs inside the support, (ci, cj, chain sign, pattern id);
//   * <H>: the list of (ci, cj, coefficient) with H_{ij} != 0 inside the support — the quadratic form of the
//     Hamiltonian restricted to S (coefficients D_g(i) summed on the host, real mode).
// Results are identical to the dense kernels up to the summation order of <H> (skipped work is exact zeros).
// One WAVE owns SPW evaluations: no workgroup barrier exists anywhere; LDS traffic of a wave is in order.
#pragma once
#include "sv_small.hpp"
#include "sv_metric_host.hpp"
#include "sv_sparse_layout.hpp"
#include "sv_wave_reduce.hpp"

namespace ovqe {

static_assert(sizeof(double2) == SP_CS_BYTES, "the layouts of sv_sparse_layout.hpp count a cos/sin entry as one double2");

// ---- building blocks of the one-wave kernels (k_sparse_vqe, k_sparse_grad, k_sparse_metric; k_sparse_hessian: see there) -------------
// A kernel is: sp_stage, then per work item a table fill, walks of the op list (sp_for_ops / sp_for_ops_down) whose bodies are the
// Givens steps below on one decoded pair, an entry loop (sp_entry_amps / sp_apply_entry) and sp_fold.  The s_waitcnt fences between
// the phases stay in the kernels: they are each kernel's own ordering argument (the gradient kernels share theirs: sp_adjoint_row).
struct SpProgram { const SpOp *opv; const uint32_t *pv; };   // the op records and pair words a walk reads: LDS (STAGE) or global memory
struct SpPair { uint32_t ci, cj; int e; bool neg; };          // a decoded pair word: the two compact indices, the table entry, the sign
struct SpRot { double c, sn; };                               // its rotation: cos, and sin with the pair's sign
struct SpAmps { double u, v; };                               // a vector's two amplitudes (slot ci, slot cj)

// STAGE: the op table and the pair words are copied to LDS once per launch, so that the chain op -> pair word -> amplitudes never
// waits for global memory (NT: the threads that copy, `lane` one of them — a workgroup of several waves puts its barrier behind the call)
template <bool STAGE, int NT = 64>
__device__ __forceinline__ SpProgram sp_stage(unsigned char *smem, size_t ops_off, size_t pairs_off, const SpOp *ops, const uint32_t *pairs,
                                              int nops, int npairs, int lane) {
    if constexpr (STAGE) {
        SpOp *lops = reinterpret_cast<SpOp *>(smem + ops_off);
        uint32_t *lpairs = reinterpret_cast<uint32_t *>(smem + pairs_off);
        for (int i = lane; i < nops; i += NT) lops[i] = ops[i];
        for (int i = lane; i < npairs; i += NT) lpairs[i] = pairs[i];
        return {lops, lpairs};
    } else {
        return {ops, pairs};
    }
}

__device__ __forceinline__ SpPair sp_decode(uint32_t pw, int tab0) {
    return {pw & 0xfffu, (pw >> 12) & 0xfffu, tab0 + (int)(pw >> 25), (pw & (1u << 24)) != 0u};
}
__device__ __forceinline__ SpRot sp_rot(const double2 *cs, const SpPair &p) {
    const double2 t = cs[p.e];
    return {t.x, p.neg ? -t.y : t.y};
}
__device__ __forceinline__ SpAmps sp_get(const double *vec, const SpPair &p) { return {vec[p.ci], vec[p.cj]}; }
__device__ __forceinline__ void sp_put(double *vec, const SpPair &p, const SpAmps &a) {
    vec[p.ci] = a.u;
    vec[p.cj] = a.v;
}
__device__ __forceinline__ double sp_signed(const SpPair &p, double x) { return p.neg ? -x : x; }

// the Givens step G of a pair, u' = c u + sigma s v, v' = c v - sigma s u, and its inverse G^T
__device__ __forceinline__ SpAmps sp_rotate(const SpRot &r, const SpAmps &a) { return {r.c * a.u + r.sn * a.v, r.c * a.v - r.sn * a.u}; }
__device__ __forceinline__ SpAmps sp_rotate_back(const SpRot &r, const SpAmps &a) { return {r.c * a.u - r.sn * a.v, r.c * a.v + r.sn * a.u}; }
// ... with the derivative of the step on top (d = sigma coeff_e for an entry of the direction's parameter, else 0; sv_hessian_host.hpp):
// t' = G t + d J psi' (psi AFTER the step)
__device__ __forceinline__ SpAmps sp_rotate_inject(const SpRot &r, double d, const SpAmps &t, const SpAmps &psi1) {
    return {r.c * t.u + r.sn * t.v + d * psi1.v, r.c * t.v - r.sn * t.u - d * psi1.u};
}
// the plain forward step on a vector in LDS
__device__ __forceinline__ void sp_rotate_pair(double *vec, const double2 *cs, const SpPair &p) {
    const SpRot r = sp_rot(cs, p);
    sp_put(vec, p, sp_rotate(r, sp_get(vec, p)));
}
// ... and on psi and one tangent t together (dk[e]: coeff_e where entry e is the direction's parameter's, else 0)
__device__ __forceinline__ void sp_tangent_pair(double *psi, double *t, const double2 *cs, const double *dk, const SpPair &p) {
    const SpRot r = sp_rot(cs, p);
    const double d = sp_signed(p, dk[p.e]);
    const SpAmps a = sp_get(psi, p), tt = sp_get(t, p);
    const SpAmps a1 = sp_rotate(r, a);
    sp_put(psi, p, a1);
    sp_put(t, p, sp_rotate_inject(r, d, tt, a1));
}

// one op: body(pair) for its pairs, STRIDE lanes apart.  The pairs of one op are disjoint; the next op may touch them from other lanes of
// this wave: the LDS unit executes a wave's DS instructions in issue order, so only the COMPILER must not reorder across ops
template <int STRIDE, class Body>
__device__ __forceinline__ void sp_op_pairs(const SpProgram &P, int o, int lane, Body &body) {
    SpOp op = P.opv[o];
    op.first = __builtin_amdgcn_readfirstlane(op.first);
    op.npairs = __builtin_amdgcn_readfirstlane(op.npairs);
    op.tab0 = __builtin_amdgcn_readfirstlane(op.tab0);
    for (int pe = lane; pe < op.npairs; pe += STRIDE) body(sp_decode(P.pv[op.first + pe], op.tab0));
    asm volatile("" ::: "memory");
}
// the ops [o0, o1) in program order, and the same ops backwards
template <int STRIDE, class Body>
__device__ __forceinline__ void sp_for_ops(const SpProgram &P, int o0, int o1, int lane, Body body) {
    for (int o = o0; o < o1; ++o) sp_op_pairs<STRIDE>(P, o, lane, body);
}
template <int STRIDE, class Body>
__device__ __forceinline__ void sp_for_ops_down(const SpProgram &P, int o0, int o1, int lane, Body body) {
    for (int o = o1 - 1; o >= o0; --o) sp_op_pairs<STRIDE>(P, o, lane, body);
}

// the cos/sin table: cs[e] = (cos, sin) of angle(record e) for e = first, first + STRIDE, ...; also(e, record) fills what else the
// kernel keeps per entry
template <int STRIDE, class Rec, class Angle, class Also>
__device__ __forceinline__ void sp_fill_table(const Rec *tab, int ntab, int first, double2 *cs, Angle angle, Also also) {
    for (int e = first; e < ntab; e += STRIDE) {
        const Rec te = tab[e];
        double sn, c;
        sincos(angle(te), &sn, &c);
        cs[e] = make_double2(c, sn);
        also(e, te);
    }
}

// one entry of the restricted Hamiltonian: the amplitudes it couples in a vector, and out[k] += H a[k] for it, for N vectors at once
// (f64 LDS atomics: out_i += H_ij a_j, out_j += H_ij a_i)
__device__ __forceinline__ SpAmps sp_entry_amps(const SpEntry &en, const double *vec) {
    const uint32_t ci = en.ij & 0xfffu, cj = (en.ij >> 12) & 0xfffu;
    return {vec[ci], vec[cj]};
}
template <int N>
__device__ __forceinline__ void sp_apply_entry(const SpEntry &en, const SpAmps (&a)[N], double *const (&out)[N]) {
    const uint32_t ci = en.ij & 0xfffu, cj = (en.ij >> 12) & 0xfffu;
    if (ci == cj) {
#pragma unroll
        for (int k = 0; k < N; ++k) __hip_atomic_fetch_add(&out[k][ci], en.c * a[k].u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    } else {   // c = 2 H_ij, the pair counted once
        const double hc = 0.5 * en.c;
#pragma unroll
        for (int k = 0; k < N; ++k) {
            __hip_atomic_fetch_add(&out[k][ci], hc * a[k].v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_add(&out[k][cj], hc * a[k].u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    }
}

// d / dtheta_k = sum over the table entries of parameter k of 2 coeff w[e]   (Rec: SmallRot or metric::TabEntry)
template <int STRIDE, class Rec>
__device__ __forceinline__ void sp_fold(const Rec *tab, int ntab, const double *w, double *gk, int tid) {
    for (int e = tid; e < ntab; e += STRIDE) {
        const Rec te = tab[e];
        if (te.pidx >= 0) __hip_atomic_fetch_add(&gk[te.pidx], 2.0 * te.coeff * w[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
}

template <int SPW, bool STAGE>
__global__ __launch_bounds__(64) void k_sparse_vqe(SparseArgs A, const double *__restrict__ theta,
                                                   const SmallRot *__restrict__ tabrots,
                                                   const SpOp *__restrict__ ops, const uint32_t *__restrict__ pairs,
                                                   const SpEntry *__restrict__ entries,
                                                   double *__restrict__ energies) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const SpVqeLds L = sp_vqe_lds(A, SPW, STAGE);
    double *st = reinterpret_cast<double *>(smem);
    double2 *cs = reinterpret_cast<double2 *>(smem + L.cs);
    const int lane = threadIdx.x;
    const SpProgram P = sp_stage<STAGE>(smem, L.ops, L.pairs, ops, pairs, A.nops, A.npairs, lane);
    // the wave's lanes are split evenly over its SPW evaluations (no index division in the inner loops)
    constexpr int LPS = 64 / SPW;
    const int s = lane / LPS, l = lane % LPS;
    double *base = st + (size_t)s * A.mpad;
    double2 *csb = cs + (size_t)s * A.ntab;
    const int64_t nwork = (A.B + SPW - 1) / SPW;
    for (int64_t w = blockIdx.x; w < nwork; w += gridDim.x) {
        const int64_t b0 = w * SPW;
        // |HF> (compact index 0) and the cos/sin table of every active pattern, per evaluation
        for (int i = lane; i < SPW * A.mpad; i += 64) st[i] = (i % A.mpad == A.hf) ? 1.0 : 0.0;
        {
            const int64_t b = b0 + s < A.B ? b0 + s : A.B - 1;
            const double *th = theta + b * A.K;
            sp_fill_table<LPS>(tabrots, A.ntab, l, csb, [&](const SmallRot &sr) { return sr.coeff * th[sr.pidx]; }, [](int, const SmallRot &) {});
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if constexpr (STAGE) {
            sp_for_ops<LPS>(P, 0, A.nops, l, [&](const SpPair &p) { sp_rotate_pair(base, csb, p); });
        } else if (A.nops > 0) {   // (a program with no active op on the support has no op record to fetch ahead)
            // op records and pair words stream from L2: the chain record -> pair word -> amplitudes of consecutive ops is
            // what bounds this kernel, so both are fetched AHEAD — the record of op o + 3 and the first pair words of ops o + 1,
            // o + 2 are in flight while op o rotates its pairs (most ops have fewer pairs than lanes: one word per lane)
            const int last = A.nops - 1;
            SpOp op1 = ops[0], op2 = ops[min(1, last)], op3 = ops[min(2, last)];
            uint32_t pw1 = l < op1.npairs ? pairs[op1.first + l] : 0u;
            uint32_t pw2 = (last >= 1 && l < op2.npairs) ? pairs[op2.first + l] : 0u;
            for (int o = 0; o < A.nops; ++o) {
                const SpOp op = op1;
                uint32_t pw = pw1;
                op1 = op2;
                pw1 = pw2;
                op2 = op3;
                op3 = ops[min(o + 3, last)];
                pw2 = (o + 2 <= last && l < op2.npairs) ? pairs[op2.first + l] : 0u;
                for (int pe = l; pe < op.npairs; pe += LPS) {
                    if (pe != l) pw = pairs[op.first + pe];
                    sp_rotate_pair(base, csb, sp_decode(pw, op.tab0));
                }
                asm volatile("" ::: "memory");
            }
        }
        double acc[SPW];
#pragma unroll
        for (int s = 0; s < SPW; ++s) acc[s] = 0.0;
#pragma unroll 4  // four entries in flight: the loop is bound by the latency of its loads, not by issue
        for (int e = lane; e < A.nent; e += 64) {
            const SpEntry en = entries[e];
            const uint32_t ci = en.ij & 0xfffu, cj = (en.ij >> 12) & 0xfffu;
#pragma unroll
            for (int s = 0; s < SPW; ++s) acc[s] += en.c * st[(size_t)s * A.mpad + ci] * st[(size_t)s * A.mpad + cj];
        }
#pragma unroll
        for (int s = 0; s < SPW; ++s) {
            const double tot = wave_sum_lane0(WaveLanes{lane}, acc[s]);   // (the tree of wave_sum: sv_wave_reduce.hpp)
            if (lane == 0 && b0 + s < A.B) energies[b0 + s] = tot + A.constant;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
}


// ---- throughput form of the circuit (round 3): rows of 32 padded 64-bit words ------------------------------------------------
// rocprofv3 counters of k_sparse_vqe<2> on the H2O workload: the LDS pipe is active 6 % of the wave cycles and bank-conflict
// cycles can be cut by a third without any change in run time; 39 % of the wave cycles are instruction issue — about 60
// instructions per op and wave (25 scalar: op records three ops ahead, loop bounds; 20 vector: unpacking the pair word,
// addresses, sign) around 4 f64 operations and 5 LDS accesses.  This form removes the bookkeeping: the program is a flat
// list of ROWS of 32 words (an op's pairs in chunks of 32, padded), one word per lane and row, everything pre-computed in it:
//   bits 0-15 byte offset of amplitude i | 16-31 byte offset of amplitude j | 32-47 byte offset of the cos/sin entry | 63 sign
// Padded lanes rotate two private spare slots behind the support by the identity entry behind the table (no branch).  Rows are
// fetched four ahead in registers; per row: one 8-byte load, three LDS reads, four f64 operations, two LDS writes.
template <int SPW, int DBG = 0>   // DBG: measurements ("sparse_dbg": 1 no sincos, 2 no circuit rows, 3 no Hamiltonian entries; 5: the wave sums by wave_sum) — a
// run-time test of A.dbg in the loop bounds cost the product kernel 12 % (0.714 -> 0.80 ms per 65 536 evaluations), hence compile time
__global__ __launch_bounds__(64) void k_sparse_vqe_rows(SparseArgs A, const double *__restrict__ theta,
                                                        const SmallRot *__restrict__ tabrots, const uint64_t *__restrict__ rows,
                                                        int nrows4, const SpEntry *__restrict__ entries,
                                                        double *__restrict__ energies) {
    static_assert(SPW == 2, "rows are built for two evaluations per wave (32 lanes each)");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const SpRowsLds L = sp_rows_lds(A, SPW);
    double *st = reinterpret_cast<double *>(smem);
    double2 *cs = reinterpret_cast<double2 *>(smem + L.cs);
    const int lane = threadIdx.x;
    constexpr int LPS = 64 / SPW;
    const int s = lane / LPS, l = lane % LPS;
    const int ntab1 = A.ntab + 1;
    unsigned char *sbase = smem + (size_t)s * A.mpad * sizeof(double);
    unsigned char *cbase = smem + L.cs + (size_t)s * ntab1 * sizeof(double2);
    const int64_t nwork = (A.B + SPW - 1) / SPW;
    const uint64_t *rp = rows + l;
    for (int64_t w = blockIdx.x; w < nwork; w += gridDim.x) {
        const int64_t b0 = w * SPW;
        uint64_t w0 = rp[0], w1 = rp[32], w2 = rp[64], w3 = rp[96];   // (the table ends with four spare rows)
        for (int i = lane; i < SPW * A.mpad; i += 64) st[i] = (i % A.mpad == A.hf) ? 1.0 : 0.0;
        {
            const int64_t b = b0 + s < A.B ? b0 + s : A.B - 1;
            const double *th = theta + b * A.K;
            for (int e = l; e < A.ntab; e += LPS) {
                const SmallRot sr = tabrots[e];
                double sn, c;
                if (DBG == 1) {
                    sn = sr.coeff * th[sr.pidx];
                    c = 1.0;
                } else {
                    sincos(sr.coeff * th[sr.pidx], &sn, &c);
                }
                cs[(size_t)s * ntab1 + e] = make_double2(c, sn);
            }
            if (l == 0) cs[(size_t)s * ntab1 + A.ntab] = make_double2(1.0, 0.0);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        auto apply = [&](uint64_t word) {
            const uint32_t lo = (uint32_t)word, hi = (uint32_t)(word >> 32);
            double *pi = reinterpret_cast<double *>(sbase + (lo & 0xffffu));
            double *pj = reinterpret_cast<double *>(sbase + (lo >> 16));
            const double2 t = *reinterpret_cast<const double2 *>(cbase + (hi & 0xffffu));
            const double sn = __hiloint2double(__double2hiint(t.y) ^ (int)(hi & 0x80000000u), __double2loint(t.y));
            const double u = *pi, v = *pj;
            *pi = t.x * u + sn * v;
            *pj = t.x * v - sn * u;
            // pairs of one row are disjoint; the next row may touch them from other lanes of this wave: the LDS unit executes a
            // wave's DS instructions in issue order, so only the COMPILER must not reorder across rows
            asm volatile("" ::: "memory");
        };
        for (int r = 0; r < (DBG == 2 ? 0 : nrows4); r += 4) {
            const uint64_t *nx = rp + (size_t)(r + 4) * 32;
            apply(w0);
            w0 = nx[0];
            apply(w1);
            w1 = nx[32];
            apply(w2);
            w2 = nx[64];
            apply(w3);
            w3 = nx[96];
        }
        double acc[SPW];
#pragma unroll
        for (int q = 0; q < SPW; ++q) acc[q] = 0.0;
        // (Measured and dropped: the next trip's entries in flight while this trip's are contracted — 0.69 ms per 65 536 against 0.67:
        // with nine waves per CU the kernel is bound by LDS instructions, ~5 per pair and 2 per entry and state at ~3 ns each per CU,
        // tools/micro/lds_atomic.hip, not by this loop's latency.  Also measured and dropped: the restricted Hamiltonian in row format
        // (lane = row, a_i once per slice of 64 rows, ONE amplitude read per entry and state instead of two, entries ordered
        // against bank conflicts): 0.673 ms against 0.675 — the entry loop's LDS reads are not what bounds THIS kernel either
        // (it streams the entries from L2; with the entries in registers they are: k_sparse_vqe_rows_shared below reads a_i once);
        // per wave and pair of evaluations ~6600 VALU, 3700 SALU, 1400 LDS instructions at 2.25 waves per SIMD.)
        // (Round 4, measured and dropped: the two states copied side by side behind the circuit (slot -> double2) so that ONE 16-byte
        // LDS read per amplitude serves both states and one address is computed instead of two — bit-identical energies, 0.885 ms
        // against 0.755: random 16-byte reads conflict more than twice as often as random 8-byte reads.  tools/exp_value_phases.py:
        // of the 0.79 ms per 65 536 evaluations through host buffers this loop is 0.40, the circuit rows 0.23, the sincos 0.03.)
#pragma unroll 4
        for (int e = lane; e < (DBG == 3 ? 0 : A.nent); e += 64) {
            const SpEntry en = entries[e];
            const uint32_t ci = en.ij & 0xfffu, cj = (en.ij >> 12) & 0xfffu;
#pragma unroll
            for (int q = 0; q < SPW; ++q) acc[q] += en.c * st[(size_t)q * A.mpad + ci] * st[(size_t)q * A.mpad + cj];
        }
#pragma unroll
        for (int q = 0; q < SPW; ++q) {
            const double tot = DBG == 5 ? wave_sum(acc[q]) : wave_sum_lane0(WaveLanes{lane}, acc[q]);
            if (lane == 0 && b0 + q < A.B) energies[b0 + q] = tot + A.constant;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
}

struct SpRowsSharedLds { size_t cs, red, bytes; };   // the 2 NW states, SSTRIDE bytes apart, are at 0
template <int NW, int SSTRIDE>
__host__ __device__ constexpr SpRowsSharedLds sp_rows_shared_lds(int ntab) {
    constexpr size_t NS = 2 * NW;
    const size_t cs = NS * SSTRIDE;                                          // [NS][ntab + 1]: the last entry is the identity
    const size_t red = cs + NS * (size_t)(ntab + 1) * sizeof(double2);     // [NW][NS] partial sums
    return {cs, red, red + (size_t)NW * NS * sizeof(double)};
}

// ---- throughput form, workgroup geometry: the restricted Hamiltonian in REGISTERS, as owner pieces ---------------------------------
// Half of k_sparse_vqe_rows<2> on the H2O workload is its entry loop: every wave streams the whole entry table from L2 (151 KB)
// for every pair of evaluations, one 16-byte load + unpacking + two address computations per entry, lane and state.  Here NW
// waves share a workgroup.  Each wave runs the circuit of ITS two evaluations exactly as above (same row table, rows four ahead,
// no barrier between rows); the 2 NW states lie side by side in LDS at the compile-time stride SSTRIDE (bytes), the cos/sin
// tables behind them.  The entries are a symmetric quadratic form, E = sum_i a_i (sum_{j in row i} c_ij a_j): the host packs them
// into OWNER PIECES (sparse_pack.hpp: up to EPR entries that share their first amplitude, either endpoint of an off-diagonal entry
// may own it, rows above EPR entries are split, tails padded with coefficient 0).  Thread t holds RPT pieces in registers for the
// whole launch — per piece the owner's byte offset, per slot the coefficient in two VGPRs and the other amplitude's byte offset,
// two to a VGPR — and after ONE barrier every wave contracts its pieces against ALL 2 NW states: per piece and state the owner's
// amplitude is read ONCE, then one ds_read_b64 and one fma per slot, t += c a_j, and acc += a_i t.  RPT (EPR + 1) reads per
// thread and state against 2 entries-per-thread before (H2O: 44 against 74, LiH: 18 against 26; profiles/owner_rows/README.md);
// the f64 operations per entry halve.  The addresses are offset + q * SSTRIDE, instruction immediates, no global traffic, no
// address arithmetic.  Partial sums of the NW waves go through LDS and are added in wave order (no floating-point atomics: the
// energy of a parameter vector depends neither on its position in the batch nor on the run).  The second barrier also frees the
// states for the next work item of the persistent loop.
// Two things the compiler needs: the stride at compile time (with a run-time stride it hoists all the addresses out of the work
// loop and spills), and the sums pinned after each slot (otherwise it finishes state 0 over all slots first and parks every
// other state's loads in scratch).  SSTRIDE is the state rounded up to 512 bytes PLUS 8: at a multiple of 512 the compiler pairs
// the reads of two states into ds_read2st64_b64, which the LDS serves at half the rate of two ds_read_b64 (8 against 2 x 2 cycles
// per wave) and in groups of 16 lanes against 32 banks, where the host's arrangement of the pieces (owners and slots that differ
// mod 32 inside aligned groups of 32 lanes) does not hold — measured on the H2O workload: 0.73 ms per 65 536 evaluations with a
// stride of 4096 (no gain over the per-wave geometry).  With + 8 every state is shifted by one slot against its neighbour: the
// same shift for all lanes of an instruction, the arrangement keeps its meaning.  DBG as k_sparse_vqe_rows.
// hc / ho: the packed tables of sparse_pack.hpp for NT = 64 NW threads — coefficients [RPT * EPR][NT]; 16-bit byte offsets
// [RPT * EPR][NT] of the slots, then [RPT][NT] of the owners.
//
// THE ITEM LOOP IS PIPELINED (profiles/pipelined_rows/README.md).  The four waves walk the work items in lock step, so
// whatever one of them waits for nothing else on the CU covers.  What an item needs from global memory is known one item ahead:
//   * table records (parameter index, coefficient) are the same for every evaluation of a launch: lane l of each half-wave holds
//     those of entries l + 32 k, k < TE, in registers from before the loop (entries beyond 32 TE — programs with more distinct
//     angles than that — keep the loads at sincos time);
//   * the theta values of item w + gridDim.x are loaded behind the last circuit row of item w, BEFORE the first barrier, and first
//     used behind the contraction, which issues no vector-memory instruction: a whole contraction hides them.  (Not earlier: vmcnt
//     retires in order and the row loop waits on it for its row words — a theta load in front of a row stalls that row.)
//   * the next item's cos/sin table is written behind the contraction and this wave's partial sums, before the second barrier,
//     into the SAME LDS region: a wave's own table is dead once its circuit is done, no other wave reads it, and a wave's DS
//     instructions execute in order.  Same sincos of the same product coeff * theta: every energy keeps its bits.  The code has
//     ONE table site: the loop is rotated so that it serves the first item of a workgroup too (then nothing precedes it);
//   * the last trip of the row loop fetches rows 0..3 again instead of the spare rows behind the table: the next item starts on
//     row words it already holds.
// The zero-fill of the states stays behind the second barrier: other waves read this wave's states in the contraction.
// What it costs is registers that live across the contraction, the kernel's pressure peak: TE records and TE theta values per lane
// (H2O 198 -> 230 VGPRs, two waves per SIMD as before; LiH 128 -> 148, three instead of four).  Measured, 65 536 evaluations: H2O
// 0.519 -> 0.484 ms, LiH 0.272 -> 0.259; the plain loop and the carried row words alone were built from a build-time switch for
// that comparison (no gain from the row words alone) and are gone.
//
// THE CONTRACTION READS ONE GROUP AHEAD (profiles/contraction_ahead/README.md).  The pins that keep the sums in state order are
// asm statements, and to the scheduler each is a barrier for memory operations too: no read of slot k + 1 moves above the fma of
// slot k.  Written slot by slot the phase is RPT (EPR + 1) times "NS reads, s_waitcnt lgkmcnt(0), NS fma": one whole LDS round
// trip per group, in series, with two (H2O) or three (LiH) waves per SIMD to cover it.  So the rotation is in the SOURCE: the
// pieces are one sequence of groups g = r (EPR + 1) + k (k = EPR: the owner read), the NS reads of group g + 1 are issued in
// front of the fma of group g, a sched_barrier(0) on either side of the arithmetic holds them there, and the compiler's own
// counted waits (lgkmcnt(14) ... (8)) let each fma go when its operand is back.  Same reads, same fma in the same order per
// state: every energy keeps its bits.  It costs the NS doubles of the group in flight: H2O 230 -> 252 VGPRs, LiH 148 -> 164,
// four registers under the steps to one wave less per SIMD (256, 168); no scratch.  (Without the pins the rotation takes 256 VGPRs
// + 256 AGPRs + 1220 bytes of scratch; with the reads and fma of a group interleaved one by one through sched_group_barrier the
// compiler reuses the registers of consumed operands, 240 / 154 VGPRs, and the kernel is no faster than the parent — measured.)
// In the rows loop the cos/sin entry of row r + 1 is read behind the amplitude reads of row r, in front of its two writes: the
// entry depends on the row word alone, and the 16-byte read leaves the chain read -> fma -> write of the next row.  The order
// of all state reads and writes is the same; no register at the peak.  Measured, 65 536 evaluations of H2O, each step against
// the one before: the contraction ahead 0.431 -> 0.422 ms (about 2 %: the LDS pipeline is busy for over half of the launch and
// shared with the rows of the CU's other workgroup, the round trips were not all that the phase waited for), the entry ahead
// 0.422 -> 0.391 (a row's chain is longest while the other workgroup contracts).  LiH 0.229 -> 0.225.
//
// THE WAVE SUMS STAY IN REGISTERS (sv_wave_reduce.hpp; profiles/wave_sums/README.md).  Behind the contraction every wave sums its
// NS = 8 accumulators over its lanes.  With wave_sum that was 8 x 6 __shfl_down steps on doubles: 96 ds_bpermute_b32, an
// s_waitcnt lgkmcnt(0) in front of each of the 48 v_add_f64, each state's total through its own exec-masked ds_write_b64 — 48 LDS
// round trips in strict series per wave and work item, all four waves at once, in front of the second barrier and through the LDS
// queue that the rows of the CU's other workgroup need.  wave_sums8 reduces the eight states TRANSPOSED on the VALU: four
// v_permlane32_swap pairs leave states 0..3 in lanes 0-31 and states 4..7 in lanes 32-63, two v_permlane16_swap pairs two states
// per row of 16 lanes, a select and a DPP row_ror:8 one state per octet, row_shl:4 / 2 / 1 finish inside the octet: 12 swaps, 8 DPP
// moves, 4 v_cndmask, 10 v_add_f64, and ONE ds_write_b64 from lanes 8 q into red[wave][q].  Every level adds the same two operands
// as the __shfl_down tree of lane 0 (addition commutes bit for bit): every energy keeps its bits.  No ds_bpermute_b32 is left in
// either instance; 250 / 162 VGPRs (the tail lies behind the register peak).  reduce(), the red layout and the wave-order addition
// of the NW partial sums are as they were.
// DBG as k_sparse_vqe_rows; 4: no theta load at all, a constant in its place (what the loads themselves cost); 5: the wave sums by
// wave_sum as before (testing build: the reference of tests/test_gpu_sparse_reduce.py, and the cost of the old tail in one build).
template <int NW, int RPT, int EPR, int SSTRIDE, int TE, int DBG = 0>
__global__ __launch_bounds__(NW * 64) void k_sparse_vqe_rows_shared(SparseArgs A, const double *__restrict__ theta,
                                                                    const SmallRot *__restrict__ tabrots, const uint64_t *__restrict__ rows,
                                                                    int nrows4, const double *__restrict__ hc, const uint16_t *__restrict__ ho,
                                                                    double *__restrict__ energies) {
    constexpr int NT = NW * 64, NS = 2 * NW, SD = SSTRIDE / 8;
    constexpr int TR = TE, TRN = TR ? TR : 1;   // table records in registers per lane
    static_assert(SSTRIDE % 8 == 0 && SSTRIDE % 512 != 0 && NS * SSTRIDE <= 65536 && (NS * SSTRIDE) % 16 == 0,
                  "state offsets are DS instruction immediates; a stride the ds_read2 forms cannot encode (see above)");
    static_assert(TE >= 0, "table records per lane");
    static_assert(NS == 8, "the transposed wave sums (wave_sums8) are built for eight states per workgroup");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int ntab1 = A.ntab + 1;
    const SpRowsSharedLds L = sp_rows_shared_lds<NW, SSTRIDE>(A.ntab);
    double2 *cs = reinterpret_cast<double2 *>(smem + L.cs);
    double *red = reinterpret_cast<double *>(smem + L.red);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = lane >> 5, l = lane & 31, my = 2 * wave + s;                // my: this half-wave's state of the workgroup
    unsigned char *sbase = smem + (size_t)my * SSTRIDE;
    double *sst = reinterpret_cast<double *>(sbase);
    double2 *csm = cs + (size_t)my * ntab1;
    unsigned char *cbase = reinterpret_cast<unsigned char *>(csm);
    // this thread's pieces: loaded once per launch
    constexpr int OPP = (EPR + 1) / 2;   // VGPRs of a piece's slot offsets
    uint32_t oi[RPT], ojj[RPT][OPP];
    double ec[RPT][EPR];
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
        oi[r] = ho[(size_t)(RPT * EPR + r) * NT + tid];
#pragma unroll
        for (int k = 0; k < EPR; ++k) ec[r][k] = hc[(size_t)(r * EPR + k) * NT + tid];
#pragma unroll
        for (int k = 0; k < OPP; ++k) {
            const uint32_t lo = ho[(size_t)(r * EPR + 2 * k) * NT + tid];
            const uint32_t hi = 2 * k + 1 < EPR ? ho[(size_t)(r * EPR + 2 * k + 1) * NT + tid] : 0u;
            ojj[r][k] = lo | (hi << 16);
        }
    }
    // ... and this lane's table records (a lane past the table holds the last record: its theta load is a valid one, nothing is
    // written for it)
    int32_t tp[TRN];
    double tc[TRN];
#pragma unroll
    for (int k = 0; k < TR; ++k) {
        const int e = l + 32 * k;
        const SmallRot sr = tabrots[e < A.ntab ? e : A.ntab - 1];
        tp[k] = sr.pidx;
        tc[k] = sr.coeff;
    }
    const int64_t nwork = (A.B + NS - 1) / NS;
    const uint64_t *rp = rows + l;
    // the parameter row of this half-wave's evaluation of work item w (the spare states of the last item run the clamped last row)
    auto theta_row = [&](int64_t w) {
        const int64_t b = w * NS + my;
        return theta + (b < A.B ? b : A.B - 1) * A.K;
    };
    auto fetch = [&](int64_t w, double (&tv)[TRN]) {
        const double *th = theta_row(w);
#pragma unroll
        for (int k = 0; k < TR; ++k) tv[k] = DBG == 4 ? 0.05 : th[tp[k]];
    };
    auto entry = [&](int e, double x) {
        double sn, c;
        if (DBG == 1) {
            sn = x;
            c = 1.0;
        } else {
            sincos(x, &sn, &c);
        }
        csm[e] = make_double2(c, sn);
    };
    auto table = [&](int64_t w, const double (&tv)[TRN]) {
#pragma unroll
        for (int k = 0; k < TR; ++k)
            if (l + 32 * k < A.ntab) entry(l + 32 * k, tc[k] * tv[k]);
        if (32 * TR < A.ntab) {
            const double *th = theta_row(w);
            for (int e = l + 32 * TR; e < A.ntab; e += 32) {
                const SmallRot sr = tabrots[e];
                entry(e, sr.coeff * (DBG == 4 ? 0.05 : th[sr.pidx]));
            }
        }
    };
    auto zero_fill = [&]() {
        for (int i = l; i < SD; i += 32) sst[i] = i == A.hf ? 1.0 : 0.0;
    };
    auto reduce = [&](int64_t b0) {   // partial sums in wave order
        if (tid < NS && b0 + tid < A.B) {
            double e = 0.0;
#pragma unroll
            for (int v = 0; v < NW; ++v) e += red[v * NS + tid];
            energies[b0 + tid] = e + A.constant;
        }
    };
    int64_t w = blockIdx.x, bprev = 0;
    if (w >= nwork) return;
    uint64_t w0 = rp[0], w1 = rp[32], w2 = rp[64], w3 = rp[96];
    double tv[TRN];
    fetch(w, tv);
    if (l == 0) csm[A.ntab] = make_double2(1.0, 0.0);   // the identity entry: nothing overwrites it
    zero_fill();
    for (bool first = true;; first = false) {
        table(w, tv);   // (behind the contraction of the item before)
        if (!first) {
            __syncthreads();   // partial sums complete; the states may be overwritten
            reduce(bprev);
            zero_fill();
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        // the cos/sin entry of a row is read ONE ROW AHEAD, behind the amplitude reads of the row before and in front of its writes:
        // it does not depend on the state (see above)
        auto cs_of = [&](uint64_t word) { return *reinterpret_cast<const double2 *>(cbase + ((uint32_t)(word >> 32) & 0xffffu)); };
        double2 tn = cs_of(w0);   // (this item's table is complete: the wait above)
        auto apply = [&](uint64_t word, uint64_t next) {
            const uint32_t lo = (uint32_t)word, hi = (uint32_t)(word >> 32);
            double *pi = reinterpret_cast<double *>(sbase + (lo & 0xffffu));
            double *pj = reinterpret_cast<double *>(sbase + (lo >> 16));
            const double2 t = tn;
            const double sn = __hiloint2double(__double2hiint(t.y) ^ (int)(hi & 0x80000000u), __double2loint(t.y));
            const double u = *pi, v = *pj;
            tn = cs_of(next);   // (the last row of an item reads the entry of row 0 from this item's table: never used)
            *pi = t.x * u + sn * v;
            *pj = t.x * v - sn * u;
            asm volatile("" ::: "memory");   // a wave's DS instructions execute in issue order (see k_sparse_vqe_rows)
        };
        auto trip = [&](const uint64_t *nx) {
            apply(w0, w1);
            w0 = nx[0];
            apply(w1, w2);
            w1 = nx[32];
            apply(w2, w3);
            w2 = nx[64];
            apply(w3, w0);
            w3 = nx[96];
        };
        if (DBG != 2) {
            for (int r = 0; r < nrows4 - 4; r += 4) trip(rp + (size_t)(r + 4) * 32);   // (fetch the four rows behind their own)
            trip(rp);   // the last trip: rows 0..3, for the next item
        }
        const int64_t wnext = w + gridDim.x;
        const bool more = wnext < nwork;
        if (more) fetch(wnext, tv);   // in flight across the barrier and the contraction
        __syncthreads();   // all 2 NW states of the workgroup are final
        double acc[NS];
#pragma unroll
        for (int q = 0; q < NS; ++q) acc[q] = 0.0;
        if (DBG != 3) {
            // the pieces as ONE sequence of read groups, g = r (EPR + 1) + k: k < EPR slot k of piece r, k = EPR its owner
            constexpr int GPP = EPR + 1, G = RPT * GPP;
            auto goff = [&](int g) -> uint32_t {
                const int r = g / GPP, k = g % GPP;
                if (k == EPR) {
                    uint32_t po = oi[r];
                    asm volatile("" : "+v"(po));   // (keeps the address arithmetic inside the loop)
                    return po;
                }
                uint32_t pk = ojj[r][k / 2];
                asm volatile("" : "+v"(pk));   // (keeps the unpacking inside the loop: EPR registers less per piece)
                return (k & 1) ? pk >> 16 : pk & 0xffffu;
            };
            double cur[NS], nxt[NS], t[NS];
            {
                const uint32_t o = goff(0);
#pragma unroll
                for (int q = 0; q < NS; ++q) cur[q] = *reinterpret_cast<const double *>(smem + o + q * SSTRIDE);
            }
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const int r = g / GPP, k = g % GPP;
                if (g + 1 < G) {   // group g + 1 in flight while group g is consumed
                    const uint32_t o = goff(g + 1);
#pragma unroll
                    for (int q = 0; q < NS; ++q) nxt[q] = *reinterpret_cast<const double *>(smem + o + q * SSTRIDE);
                }
                __builtin_amdgcn_sched_barrier(0);   // (the reads stay in front of this group's arithmetic)
                if (k < EPR) {
#pragma unroll
                    for (int q = 0; q < NS; ++q) t[q] = k ? fma(ec[r][k], cur[q], t[q]) : ec[r][k] * cur[q];
#pragma unroll
                    for (int q = 0; q < NS; ++q) asm volatile("" : "+v"(t[q]));
                } else {
#pragma unroll
                    for (int q = 0; q < NS; ++q) acc[q] = fma(cur[q], t[q], acc[q]);
#pragma unroll
                    for (int q = 0; q < NS; ++q) asm volatile("" : "+v"(acc[q]));
                }
                __builtin_amdgcn_sched_barrier(0);   // (... and the next group's reads behind it: ONE group ahead, not more)
                if (g + 1 < G) {
#pragma unroll
                    for (int q = 0; q < NS; ++q) cur[q] = nxt[q];
                }
            }
        }
        if constexpr (DBG == 5) {
#pragma unroll
            for (int q = 0; q < NS; ++q) {
                const double tot = wave_sum(acc[q]);
                if (lane == 0) red[wave * NS + q] = tot;
            }
        } else {
            const double z = wave_sums8(WaveLanes{lane}, acc);   // lane 8 q: the total of state q
            if ((lane & 7) == 0) red[wave * NS + (lane >> 3)] = z;
        }
        bprev = w * NS;
        if (!more) break;
        w = wnext;
    }
    __syncthreads();
    reduce(bprev);
}

// ---- latency form (round 3): ONE evaluation per workgroup of NT threads ---------------------------------------------------------
// What scipy's one-evaluation-per-call optimisers see.  rocprofv3: the single-wave kernel above takes 45 us per H2O evaluation
// — 26 us of it its wave walking the 9443 entries of the restricted Hamiltonian four loads at a time, the rest 140 ops of ~60
// instructions plus staging.  Here the workgroup's NT threads prepare everything in parallel (state, ONE sincos per thread) and
// pull the Hamiltonian's entries into REGISTERS while wave 0 runs the circuit — rows of 64 padded words straight from memory,
// eight rows ahead — then all waves contract their entries against the state in LDS.
template <int NT, int EPT>
__global__ __launch_bounds__(NT) void k_sparse_vqe_wg(SparseArgs A, const double *__restrict__ theta,
                                                      const SmallRot *__restrict__ tabrots, const uint64_t *__restrict__ rows,
                                                      int nrows8, const SpEntry *__restrict__ entries,
                                                      double *__restrict__ energies) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double *st = reinterpret_cast<double *>(smem);
    double2 *cs = reinterpret_cast<double2 *>(smem + sp_rows_lds(A, 1).cs);
    __shared__ double2 red[NT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#ifdef OVQE_TESTING
    uint64_t stamp[6] = {};   // "sparse_dbg" = 9: phase times of the first evaluation of workgroup 0 (s_memrealtime ticks of 10 ns)
#define OVQE_STAMP(k) do { if (A.dbg == 9) stamp[k] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define OVQE_STAMP(k) do { } while (0)
#endif
    for (int64_t b = blockIdx.x; b < A.B; b += gridDim.x) {
        OVQE_STAMP(0);
        const double *th = theta + b * A.K;
        // Hamiltonian entries of this thread: in flight from here on
        SpEntry ent[EPT];
#pragma unroll
        for (int k = 0; k < EPT; ++k) ent[k] = entries[min(tid + k * NT, A.nent - 1)];
        uint64_t w[8];
        const uint64_t *rp = rows + lane;
        if (wave == 0) {
#pragma unroll
            for (int k = 0; k < 8; ++k) w[k] = rp[k * 64];          // (the table ends with eight spare rows)
        }
        for (int i = tid; i < A.mpad; i += NT) st[i] = i == A.hf ? 1.0 : 0.0;
        for (int e = tid; e < A.ntab; e += NT) {
            const SmallRot sr = tabrots[e];
            double sn, c;
            sincos(sr.coeff * th[sr.pidx], &sn, &c);
            cs[e] = make_double2(c, sn);
        }
        if (tid == 0) cs[A.ntab] = make_double2(1.0, 0.0);
        OVQE_STAMP(1);
        __syncthreads();
        OVQE_STAMP(2);
        if (wave == 0) {
            auto apply = [&](uint64_t word) {
                const uint32_t lo = (uint32_t)word, hi = (uint32_t)(word >> 32);
                double *pi = reinterpret_cast<double *>(smem + (lo & 0xffffu));
                double *pj = reinterpret_cast<double *>(smem + (lo >> 16));
                const double2 t = *reinterpret_cast<const double2 *>(reinterpret_cast<const unsigned char *>(cs) + (hi & 0xffffu));
                const double sn = __hiloint2double(__double2hiint(t.y) ^ (int)(hi & 0x80000000u), __double2loint(t.y));
                const double u = *pi, v = *pj;
                *pi = t.x * u + sn * v;
                *pj = t.x * v - sn * u;
                asm volatile("" ::: "memory");   // a wave's DS instructions execute in issue order (see k_sparse_vqe)
            };
            for (int r = 0; r < nrows8; r += 8) {
                const uint64_t *nx = rp + (size_t)(r + 8) * 64;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    apply(w[k]);
                    w[k] = nx[k * 64];
                }
            }
        }
        OVQE_STAMP(3);
        __syncthreads();
        OVQE_STAMP(4);
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < EPT; ++k)
            if (tid + k * NT < A.nent) acc += ent[k].c * st[ent[k].ij & 0xfffu] * st[(ent[k].ij >> 12) & 0xfffu];
        for (int e = tid + EPT * NT; e < A.nent; e += NT) {       // (restricted Hamiltonians beyond EPT x NT entries)
            const SpEntry en = entries[e];
            acc += en.c * st[en.ij & 0xfffu] * st[(en.ij >> 12) & 0xfffu];
        }
        const double2 tot = block_sum<NT>(make_double2(acc, 0.0), red);
        if (tid == 0) energies[b] = tot.x + A.constant;
#ifdef OVQE_TESTING
        if (A.dbg == 9 && tid == 0 && blockIdx.x == 0 && b == 0) {
            stamp[5] = __builtin_amdgcn_s_memrealtime();
            printf("k_sparse_vqe_wg phases (10-ns ticks): prologue %llu, barrier %llu, circuit (wave 0) %llu, barrier %llu, <H> + reduce %llu; rows %d entries %d\n",
                   (unsigned long long)(stamp[1] - stamp[0]), (unsigned long long)(stamp[2] - stamp[1]), (unsigned long long)(stamp[3] - stamp[2]),
                   (unsigned long long)(stamp[4] - stamp[3]), (unsigned long long)(stamp[5] - stamp[4]), nrows8, A.nent);
        }
#endif
    }
#undef OVQE_STAMP
}

// ---- exact gradient on the compact support (round 3) ---------------------------------------------------------------------
// E(theta) and dE/dtheta_k for ALL K parameters of one parameter vector per wave, in ONE launch: forward circuit as above,
// lambda = H psi from the restricted Hamiltonian's entries (f64 LDS atomics: lambda_i += H_ij a_j, lambda_j += H_ij a_i),
// then the ops BACKWARDS on psi and lambda together — per pair g = lambda_i psi_j - lambda_j psi_i on the states after the op,
// w[table entry] += +-g, both states rotated back — and dE/dtheta_k = sum over the table entries of parameter k of
// 2 coeff w.  (The adjoint method of ovqe_energy_gradient's streaming and sector paths on the support: the streaming form
// needs ~6 launches per generator — H2O: 1.6 ms for 140 derivatives.)
//
// ONE ROW BODY, sp_adjoint_row, for the five kernels below: one wave, one parameter vector, the wave's own psi, lambda, cos/sin table,
// w and gk in LDS.  What a kernel adds — where its scalars go, what else it adds to lambda — is the functor `between`, which runs
// between "lambda = H psi" and the backward walk and gets the lane sum of <psi|H|psi> (wave_sum: the total is lane 0's).  The contract:
//   FENCES.  A wave's LDS instructions execute in issue order, and s_waitcnt lgkmcnt(0) completes them.  The body's fences: (1) behind
//   the zeroing and the table, before the forward walk reads them; (2) behind `between`, before the backward walk reads lambda: it
//   completes the atomics of lambda = H psi and whatever `between` issued last; (3) behind the backward walk: the atomics on w, before
//   the fold reads it; (4) behind the fold: the atomics on gk, before they are read; (5) behind the store, before the next row zeroes
//   the arrays.  `between` puts its OWN fence in front of every phase that reads lambda or writes it other than by atomics — the first
//   such phase needs one too, for the atomics of lambda = H psi — and between a zeroing and atomics on what was zeroed.
//   BARRIERS.  None in the body, none in `between`.  The batch kernels (sp_batch_rows) have ONE, behind the staging; every wave reaches
//   it, also a wave that owns no row, and it is outside the row loop (the waves of a workgroup finish their rows at different times).
//   No wave touches another wave's region.
//   BITS.  Every scalar of a row is summed in a fixed order — each lane its elements e or i = lane (mod 64) in rising order, then
//   wave_sum's tree — so equal rows give equal bits wherever they sit in a batch and whatever the geometry.  The order of the atomic
//   additions is not fixed: the gradient reproduces to rounding.
template <class Between>
__device__ __forceinline__ void sp_adjoint_row(const SparseArgs &A, const SpProgram &P, int lane, double *psi, double *lam, double2 *cs,
                                               double *w, double *gk, const SmallRot *__restrict__ tabrots,
                                               const SpEntry *__restrict__ entries, const double *__restrict__ th, double *__restrict__ grad,
                                               Between between) {
    for (int i = lane; i < A.mpad; i += 64) {
        psi[i] = i == A.hf ? 1.0 : 0.0;
        lam[i] = 0.0;
    }
    sp_fill_table<64>(tabrots, A.ntab, lane, cs, [&](const SmallRot &sr) { return sr.coeff * th[sr.pidx]; },
                      [&](int e, const SmallRot &) { w[e] = 0.0; });
    for (int k = lane; k < A.K; k += 64) gk[k] = 0.0;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    // forward
    sp_for_ops<64>(P, 0, A.nops, lane, [&](const SpPair &p) { sp_rotate_pair(psi, cs, p); });
    // lambda = H psi, E = <psi|lambda>: the entries from global memory — in a batch every wave reads the same records, they stay in L2
    double acc = 0.0;
#pragma unroll 4
    for (int e = lane; e < A.nent; e += 64) {
        const SpEntry en = entries[e];
        const SpAmps a = sp_entry_amps(en, psi);
        acc += en.c * a.u * a.v;
        sp_apply_entry(en, {a}, {lam});
    }
    between(wave_sum(acc));
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    // backward: the pair's weight g on the states after the op, then both states rotated back
    sp_for_ops_down<64>(P, 0, A.nops, lane, [&](const SpPair &p) {
        const SpRot r = sp_rot(cs, p);
        const SpAmps a = sp_get(psi, p), l = sp_get(lam, p);
        const double g = l.u * a.v - l.v * a.u;
        __hip_atomic_fetch_add(&w[p.e], sp_signed(p, g), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        sp_put(psi, p, sp_rotate_back(r, a));
        sp_put(lam, p, sp_rotate_back(r, l));
    });
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    sp_fold<64>(tabrots, A.ntab, w, gk, lane);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    for (int k = lane; k < A.K; k += 64) grad[k] = gk[k];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

template <bool STAGE>
__global__ __launch_bounds__(64) void k_sparse_grad(SparseArgs A, const double *__restrict__ theta, const SmallRot *__restrict__ tabrots,
                                                    const SpOp *__restrict__ ops, const uint32_t *__restrict__ pairs,
                                                    const SpEntry *__restrict__ entries, double *__restrict__ energies,
                                                    double *__restrict__ grads) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const SpGradLds L = sp_grad_lds(A, STAGE);
    double *psi = reinterpret_cast<double *>(smem);
    double *lam = reinterpret_cast<double *>(smem + L.lam);
    double2 *cs = reinterpret_cast<double2 *>(smem + L.cs);
    double *w = reinterpret_cast<double *>(smem + L.w);
    double *gk = reinterpret_cast<double *>(smem + L.gk);
    const int lane = threadIdx.x;
    const SpProgram P = sp_stage<STAGE>(smem, L.ops, L.pairs, ops, pairs, A.nops, A.npairs, lane);
    for (int64_t b = blockIdx.x; b < A.B; b += gridDim.x)
        sp_adjoint_row(A, P, lane, psi, lam, cs, w, gk, tabrots, entries, theta + b * A.K, grads + b * A.K, [&](double etot) {
            if (lane == 0) energies[b] = etot + A.constant;
        });
}

// THE BATCH FRAME of the four kernels below: workgroups of NW waves, wave v of workgroup g takes the rows g NW + v, + gridDim.x NW, ...
// What is the same for every row — the op records and the pair words — is staged ONCE per workgroup (STAGE) or read from global memory;
// what a row owns is the wave's private region of the layout Layout(A, NW, STAGE) (sv_sparse_layout.hpp: sp_grad_batch_lds, or
// sp_spread_batch_lds with its third array), psi at its start.  The kernel's functor gets the row (SpRow), the layout and the lane sum
// of <psi|H|psi>, and keeps the contract above.
struct SpRow { int64_t b; int lane; double *psi, *lam; unsigned char *mine; };   // row b of the batch; `mine`: the wave's region
template <int NW, bool STAGE, auto Layout, class Between>
__device__ __forceinline__ void sp_batch_rows(const SparseArgs &A, const double *__restrict__ theta, const SmallRot *__restrict__ tabrots,
                                              const SpOp *__restrict__ ops, const uint32_t *__restrict__ pairs,
                                              const SpEntry *__restrict__ entries, double *__restrict__ grads, Between between) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const auto L = Layout(A, NW, STAGE);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const SpProgram P = sp_stage<STAGE, NW * 64>(smem, L.ops, L.pairs, ops, pairs, A.nops, A.npairs, (int)threadIdx.x);
    __syncthreads();
    unsigned char *mine = smem + (size_t)wave * L.stride;
    double *psi = reinterpret_cast<double *>(mine);
    double *lam = reinterpret_cast<double *>(mine + L.lam);
    double2 *cs = reinterpret_cast<double2 *>(mine + L.cs);
    double *w = reinterpret_cast<double *>(mine + L.w);
    double *gk = reinterpret_cast<double *>(mine + L.gk);
    for (int64_t b = (int64_t)blockIdx.x * NW + wave; b < A.B; b += (int64_t)gridDim.x * NW)
        sp_adjoint_row(A, P, lane, psi, lam, cs, w, gk, tabrots, entries, theta + b * A.K, grads + b * A.K,
                       [&](double etot) { between(SpRow{b, lane, psi, lam, mine}, L, etot); });
}

// the deflation phase: d_r = <D_r|psi>, lambda += beta_r d_r D_r, returns sum_r beta_r d_r^2, with real rows D[r][0..mpad) in global
// memory (the stored vectors restricted to the support, k_deflate_gather; every wave reads the same rows, they stay in L2 as the
// Hamiltonian's entries do).  Every lane sums its slots i = lane (mod 64) of a row, wave_sum adds the lanes in its fixed tree, lane 0's
// total goes to all lanes, and every lane adds to its own lambda slots: plain LDS read-modify-writes, so the caller's fence goes in front.
__device__ __forceinline__ double sp_deflation_phase(const SparseArgs &A, const SpRow &R, const double *__restrict__ D,
                                                     const DeflRow *__restrict__ drows, int nrows, double *__restrict__ dvals) {
    double pen = 0.0;
    for (int r = 0; r < nrows; ++r) {
        const DeflRow dr = drows[r];
        const double *row = D + (size_t)dr.src * A.mpad;
        double dacc = 0.0;
        for (int i = R.lane; i < A.mpad; i += 64) dacc = fma(row[i], R.psi[i], dacc);
        const double d = __shfl(wave_sum(dacc), 0, 64);
        const double c = dr.beta * d;
        for (int i = R.lane; i < A.mpad; i += 64) R.lam[i] = fma(c, row[i], R.lam[i]);
        pen = fma(c, d, pen);
        if (R.lane == 0) dvals[R.b * nrows + r] = d;
    }
    return pen;
}

// the observables phase: o_m = <psi|O_m|psi> + constant_m, lambda += g_m O_m psi with g_m = linear_m + 2 quad_m (o_m - target_m), returns
// pen + sum_m [linear_m o_m + quad_m (o_m - target_m)^2].  Every O_m restricted to the support is one more SpEntry stream of the kind the
// Hamiltonian's is (sv_constrain_host.hpp: one rule for both), all of them one concatenated array in global memory, recs[m] naming the
// range and the weights.  Per observable: pass one over its entries sums c a_u a_v in registers (no LDS write), wave_sum adds the lanes
// in its fixed tree, lane 0's total goes to all lanes; g is then the same in every lane, and where it is not zero pass two applies the
// same entries to lambda with their coefficients scaled by g (f64 LDS atomics, as lambda = H psi).  Two passes instead of a third LDS
// array: the observables take no LDS.  The caller's fence goes in front (pass two follows read-modify-writes of lambda).
__device__ __forceinline__ double sp_observables_phase(const SpRow &R, const SpEntry *__restrict__ oentries, const ConRec *__restrict__ recs,
                                                       int nobs, double *__restrict__ values, double pen) {
    for (int m = 0; m < nobs; ++m) {
        const ConRec rec = recs[m];
        const SpEntry *oe = oentries + rec.first;
        double oacc = 0.0;
#pragma unroll 1   // (unrolled by four the kernel takes 95 VGPRs, five waves per SIMD; so 79, the six of k_sparse_vqd_batch: profiles/constraints)
        for (int e = R.lane; e < rec.count; e += 64) {
            const SpEntry en = oe[e];
            const SpAmps a = sp_entry_amps(en, R.psi);
            oacc += en.c * a.u * a.v;
        }
        const double o = __shfl(wave_sum(oacc), 0, 64) + rec.constant;
        if (R.lane == 0) values[R.b * nobs + m] = o;
        const double dev = o - rec.target;
        const double g = rec.linear + 2.0 * rec.quad * dev;
        pen = fma(rec.linear, o, pen);
        pen = fma(rec.quad * dev, dev, pen);
        if (g != 0.0) {   // (wave-uniform: o was broadcast)
#pragma unroll 4
            for (int e = R.lane; e < rec.count; e += 64) {
                SpEntry en = oe[e];
                en.c *= g;
                sp_apply_entry(en, {sp_entry_amps(en, R.psi)}, {R.lam});
            }
        }
    }
    return pen;
}

// ... for a BATCH of parameter vectors (ovqe_energy_gradient_batch): the frame and nothing else.
template <int NW, bool STAGE>
__global__ __launch_bounds__(NW * 64) void k_sparse_grad_batch(SparseArgs A, const double *__restrict__ theta,
                                                               const SmallRot *__restrict__ tabrots, const SpOp *__restrict__ ops,
                                                               const uint32_t *__restrict__ pairs, const SpEntry *__restrict__ entries,
                                                               double *__restrict__ energies, double *__restrict__ grads) {
    sp_batch_rows<NW, STAGE, &sp_grad_batch_lds>(A, theta, tabrots, ops, pairs, entries, grads, [&](const SpRow &R, const auto &, double etot) {
        if (R.lane == 0) energies[R.b] = etot + A.constant;
    });
}

// ... and DEFLATED (ovqe_deflated_gradient_batch): C = <psi|H|psi> + sum_r beta_r d_r^2, d_r = <D_r|psi>.  The penalty is the rank-nrows
// operator sum_r beta_r |D_r><D_r| beside H: the deflation phase behind the fence that completes the contraction's atomics.  The
// layout is sp_grad_batch_lds unchanged (the rows take no LDS).
template <int NW, bool STAGE>
__global__ __launch_bounds__(NW * 64) void k_sparse_vqd_batch(SparseArgs A, const double *__restrict__ theta,
                                                              const SmallRot *__restrict__ tabrots, const SpOp *__restrict__ ops,
                                                              const uint32_t *__restrict__ pairs, const SpEntry *__restrict__ entries,
                                                              const double *__restrict__ D, const DeflRow *__restrict__ drows, int nrows,
                                                              double *__restrict__ costs, double *__restrict__ energies,
                                                              double *__restrict__ grads, double *__restrict__ dvals) {
    sp_batch_rows<NW, STAGE, &sp_grad_batch_lds>(A, theta, tabrots, ops, pairs, entries, grads, [&](const SpRow &R, const auto &, double etot) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        const double pen = sp_deflation_phase(A, R, D, drows, nrows, dvals);
        if (R.lane == 0) {
            const double e = etot + A.constant;
            energies[R.b] = e;
            costs[R.b] = e + pen;
        }
    });
}

// ... and with OBSERVABLES beside H (ovqe_constrained_gradient_batch): C = E + sum_m [linear_m o_m + quad_m (o_m - target_m)^2] + the
// deflation penalty, o_m = <psi|O_m|psi> + constant_m.  For a cost f(E, o_1 .. o_M) the adjoint vector is lambda = H psi + sum_m
// (df/do_m) O_m psi: k_sparse_vqd_batch's functor with the observables phase behind the fence that completes the deflation phase's
// read-modify-writes of lambda.  The layout stays sp_grad_batch_lds.
template <int NW, bool STAGE>
__global__ __launch_bounds__(NW * 64) void k_sparse_constrained_batch(SparseArgs A, const double *__restrict__ theta,
                                                                      const SmallRot *__restrict__ tabrots, const SpOp *__restrict__ ops,
                                                                      const uint32_t *__restrict__ pairs, const SpEntry *__restrict__ entries,
                                                                      const double *__restrict__ D, const DeflRow *__restrict__ drows, int nrows,
                                                                      const SpEntry *__restrict__ oentries, const ConRec *__restrict__ recs,
                                                                      int nobs, double *__restrict__ costs, double *__restrict__ energies,
                                                                      double *__restrict__ grads, double *__restrict__ dvals,
                                                                      double *__restrict__ values) {
    sp_batch_rows<NW, STAGE, &sp_grad_batch_lds>(A, theta, tabrots, ops, pairs, entries, grads, [&](const SpRow &R, const auto &, double etot) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        double pen = sp_deflation_phase(A, R, D, drows, nrows, dvals);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        pen = sp_observables_phase(R, oentries, recs, nobs, values, pen);
        if (R.lane == 0) {
            const double e = etot + A.constant;
            energies[R.b] = e;
            costs[R.b] = e + pen;
        }
    });
}

// ... and with the SPREAD of the energy (ovqe_spread_gradient_batch): S = ||(H - omega) psi||^2, omega the caller's per row or — omega
// null — the row's own E, where S is the energy variance; cost = w_energy E + w_spread S with its exact gradient at fixed omega.  The
// adjoint vector is lambda = w_energy H psi + w_spread (H - omega)^2 psi: a third private array mu (sp_spread_batch_lds) and, everything
// real,
//     sigma = lambda + s psi, s = constant - omega, in place, and mu = 0;  S = sum sigma_i^2;  mu = H sigma (the entry loop again, sigma
//     the source);  lambda <- w_energy (sigma - s psi) + w_spread (mu + s sigma)
// each behind a fence that completes the phase before it (mu is zeroed in the sigma pass: a fence before the atomics on it).  The host
// launches the kernel only where the restricted entries are H on the support (spread::exactness, sv_spread_host.hpp).
template <int NW, bool STAGE>
__global__ __launch_bounds__(NW * 64) void k_sparse_spread_batch(SparseArgs A, const double *__restrict__ theta,
                                                                 const SmallRot *__restrict__ tabrots, const SpOp *__restrict__ ops,
                                                                 const uint32_t *__restrict__ pairs, const SpEntry *__restrict__ entries,
                                                                 const double *__restrict__ omega, double w_energy, double w_spread,
                                                                 double *__restrict__ costs, double *__restrict__ energies,
                                                                 double *__restrict__ spreads, double *__restrict__ grads) {
    sp_batch_rows<NW, STAGE, &sp_spread_batch_lds>(A, theta, tabrots, ops, pairs, entries, grads, [&](const SpRow &R, const auto &L, double etot) {
        double *psi = R.psi, *lam = R.lam, *mu = reinterpret_cast<double *>(R.mine + L.mu);
        const double energy = __shfl(etot, 0, 64) + A.constant;
        const double s = A.constant - (omega ? omega[R.b] : energy);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        // sigma = (H - omega) psi in place of lambda, S = <sigma|sigma>
        double sacc = 0.0;
        for (int i = R.lane; i < A.mpad; i += 64) {
            const double sg = fma(s, psi[i], lam[i]);
            lam[i] = sg;
            mu[i] = 0.0;
            sacc = fma(sg, sg, sacc);
        }
        const double stot = wave_sum(sacc);
        if (R.lane == 0) {
            energies[R.b] = energy;
            spreads[R.b] = stot;
            costs[R.b] = w_energy * energy + w_spread * stot;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        // mu = H sigma
#pragma unroll 4
        for (int e = R.lane; e < A.nent; e += 64) {
            const SpEntry en = entries[e];
            sp_apply_entry(en, {sp_entry_amps(en, lam)}, {mu});
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        // lambda = w_energy H psi + w_spread (H - omega) sigma
        for (int i = R.lane; i < A.mpad; i += 64) {
            const double sg = lam[i];
            lam[i] = w_energy * (sg - s * psi[i]) + w_spread * fma(s, sg, mu[i]);
        }
    });
}

// ... and with ONE parameter vector per workgroup (latency form, as k_sparse_vqe_wg): all threads prepare and hold the restricted
// Hamiltonian's entries in registers, wave 0 runs the circuit forwards over rows of 64 padded words, all waves form
// E = <psi|H|psi> and lambda = H psi (f64 LDS atomics), wave 0 walks the rows BACKWARDS on psi and lambda — per row
// g = lambda_i psi_j - lambda_j psi_i summed over the wave by DPP row operations when the row has one cos/sin entry (the rows of a
// JW excitation do, their padded lanes carry it too), by LDS atomics otherwise — and all threads fold w into dE/dtheta.
template <int NT, int EPT>
__global__ __launch_bounds__(NT) void k_sparse_grad_wg(SparseArgs A, const double *__restrict__ theta, const SmallRot *__restrict__ tabrots,
                                                       const uint64_t *__restrict__ rows, int nrows8, const SpEntry *__restrict__ entries,
                                                       double *__restrict__ energies, double *__restrict__ grads) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const SpGradWgLds L = sp_grad_wg_lds(A);
    double *psi = reinterpret_cast<double *>(smem);
    double *lam = reinterpret_cast<double *>(smem + L.lam);
    double2 *cs = reinterpret_cast<double2 *>(smem + L.cs);
    double *w = reinterpret_cast<double *>(smem + L.w);
    double *gk = reinterpret_cast<double *>(smem + L.gk);
    __shared__ double2 red[NT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t lam_off = (uint32_t)L.lam;
    for (int64_t b = blockIdx.x; b < A.B; b += gridDim.x) {
        const double *th = theta + b * A.K;
        SpEntry ent[EPT];
#pragma unroll
        for (int k = 0; k < EPT; ++k) ent[k] = entries[min(tid + k * NT, A.nent - 1)];
        uint64_t wd[8];
        const uint64_t *rp = rows + lane;
        if (wave == 0) {
#pragma unroll
            for (int k = 0; k < 8; ++k) wd[k] = rp[k * 64];
        }
        for (int i = tid; i < A.mpad; i += NT) {
            psi[i] = i == A.hf ? 1.0 : 0.0;
            lam[i] = 0.0;
        }
        for (int e = tid; e < A.ntab; e += NT) {
            const SmallRot sr = tabrots[e];
            double sn, c;
            sincos(sr.coeff * th[sr.pidx], &sn, &c);
            cs[e] = make_double2(c, sn);
            w[e] = 0.0;
        }
        if (tid == 0) {
            cs[A.ntab] = make_double2(1.0, 0.0);
            w[A.ntab] = 0.0;
        }
        for (int k = tid; k < A.K; k += NT) gk[k] = 0.0;
        __syncthreads();
        if (wave == 0) {   // forward
            for (int r = 0; r < nrows8; r += 8) {
                const uint64_t *nx = rp + (size_t)(r + 8) * 64;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const uint32_t lo = (uint32_t)wd[k], hi = (uint32_t)(wd[k] >> 32);
                    double *pi = reinterpret_cast<double *>(smem + (lo & 0xffffu));
                    double *pj = reinterpret_cast<double *>(smem + (lo >> 16));
                    const double2 t = *reinterpret_cast<const double2 *>(reinterpret_cast<const unsigned char *>(cs) + (hi & 0xffffu));
                    const double sn = __hiloint2double(__double2hiint(t.y) ^ (int)(hi & 0x80000000u), __double2loint(t.y));
                    const double u = *pi, v = *pj;
                    *pi = t.x * u + sn * v;
                    *pj = t.x * v - sn * u;
                    asm volatile("" ::: "memory");
                    wd[k] = nx[k * 64];
                }
            }
            // the last eight rows, for the way back (the spare rows behind the table were fetched last)
#pragma unroll
            for (int k = 0; k < 8; ++k) wd[k] = rp[(size_t)(nrows8 - 1 - k) * 64];
        }
        __syncthreads();
        double acc = 0.0;
        auto entry = [&](const SpEntry &en) {   // (sp_entry_amps / sp_apply_entry spelled out: this kernel sits at its register cap with spills,
            // and its allocation moved with the helpers — 8 bytes more scratch, or 0.9 % on the call)
            const uint32_t ci = en.ij & 0xfffu, cj = (en.ij >> 12) & 0xfffu;
            const double ai = psi[ci], aj = psi[cj];
            acc += en.c * ai * aj;
            if (ci == cj) {
                __hip_atomic_fetch_add(&lam[ci], en.c * ai, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            } else {   // c = 2 H_ij, the pair counted once
                __hip_atomic_fetch_add(&lam[ci], 0.5 * en.c * aj, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_fetch_add(&lam[cj], 0.5 * en.c * ai, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        };
#pragma unroll
        for (int k = 0; k < EPT; ++k)
            if (tid + k * NT < A.nent) entry(ent[k]);
        for (int e = tid + EPT * NT; e < A.nent; e += NT) entry(entries[e]);
        const double2 tot = block_sum<NT>(make_double2(acc, 0.0), red);   // (its barriers also complete lambda)
        if (tid == 0) energies[b] = tot.x + A.constant;
        if (wave == 0) {   // backward: rows nrows8 - 1 ... 0 (the rows of one op are independent of each other)
            for (int r = nrows8 - 1; r >= 0; r -= 8) {
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const uint32_t lo = (uint32_t)wd[k], hi = (uint32_t)(wd[k] >> 32);
                    const uint32_t oi = lo & 0xffffu, oj = lo >> 16, oe = hi & 0xffffu;
                    double *pi = reinterpret_cast<double *>(smem + oi), *pj = reinterpret_cast<double *>(smem + oj);
                    double *li = reinterpret_cast<double *>(smem + lam_off + oi), *lj = reinterpret_cast<double *>(smem + lam_off + oj);
                    const double2 t = *reinterpret_cast<const double2 *>(reinterpret_cast<const unsigned char *>(cs) + oe);
                    const bool neg = (hi & 0x80000000u) != 0u;
                    const double sn = neg ? -t.y : t.y;
                    const double u1 = *pi, v1 = *pj, lu = *li, lv = *lj;
                    const double g = lu * v1 - lv * u1, gs = neg ? -g : g;
                    const uint32_t oe0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)oe);
                    if (__all(oe == oe0)) {
                        const double rowsum = sec_wave_sum63(gs);
                        if (lane == 63) w[oe0 >> 4] += rowsum;
                    } else {
                        __hip_atomic_fetch_add(&w[oe >> 4], gs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                    *pi = t.x * u1 - sn * v1;
                    *pj = t.x * v1 + sn * u1;
                    *li = t.x * lu - sn * lv;
                    *lj = t.x * lv + sn * lu;
                    asm volatile("" ::: "memory");
                    const int nr = r - 8 - k;
                    wd[k] = rp[(size_t)max(nr, 0) * 64];
                }
            }
        }
        __syncthreads();
        sp_fold<NT>(tabrots, A.ntab, w, gk, tid);
        __syncthreads();
        for (int k = tid; k < A.K; k += NT) grads[b * A.K + k] = gk[k];
        __syncthreads();
    }
}

// ---- tangent vectors of the ansatz state on the compact support (ovqe_metric_tensor, path 1) -------------------------------------------
// T_k = d psi / d theta_k for ALL K parameters of one parameter vector in one launch: workgroup (one wave) k carries psi and ONE tangent
// t through the pair lists of the metric's own compact program (sv_metric_host.hpp: pair words as above, one table entry per distinct
// angle, constant angles and offsets kept).  A pair with table entry e = (c, s), sign sigma does u' = c u + sigma s v, v' = c v - sigma s u
// on both vectors; when entry e belongs to parameter k the derivative of that Givens rotation is added on top, t_i += coeff_e sigma v',
// t_j -= coeff_e sigma u' (psi AFTER the rotation).  The pairs of one op are disjoint and a wave's DS instructions execute in issue
// order: no atomic, no barrier, and the same bits from call to call.  Until the first op that holds an entry of parameter k (first_op, from
// the host) t is zero and psi rotates alone.  The finished tangent goes to column k of the index-major store (row i = compact index,
// wpad columns): the Gram kernel of the density matrices reads that layout as it stands.
template <bool STAGE>
__global__ __launch_bounds__(64) void k_sparse_metric(SpMetricArgs A, const double *__restrict__ theta, const metric::TabEntry *__restrict__ tab,
                                                      const metric::Op *__restrict__ ops, const uint32_t *__restrict__ pairs,
                                                      const int32_t *__restrict__ first_op, double *__restrict__ store) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const SpMetricLds L = sp_metric_lds(A, STAGE);
    double *psi = reinterpret_cast<double *>(smem);
    double *t = reinterpret_cast<double *>(smem + L.t);
    double2 *cs = reinterpret_cast<double2 *>(smem + L.cs);
    double *dk = reinterpret_cast<double *>(smem + L.dk);
    const int lane = threadIdx.x;
    const SpProgram P = sp_stage<STAGE>(smem, L.ops, L.pairs, ops, pairs, A.nops, A.npairs, lane);
    for (int k = blockIdx.x; k < A.K; k += gridDim.x) {
        for (int i = lane; i < A.mpad; i += 64) {
            psi[i] = i == A.hf ? 1.0 : 0.0;
            t[i] = 0.0;
        }
        sp_fill_table<64>(tab, A.ntab, lane, cs,
                          [&](const metric::TabEntry &te) { return te.phi0 + (te.pidx >= 0 ? te.coeff * theta[te.pidx] : 0.0); },
                          [&](int e, const metric::TabEntry &te) { dk[e] = te.pidx == k ? te.coeff : 0.0; });
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        int o1 = first_op[k];
        o1 = __builtin_amdgcn_readfirstlane(o1 < A.nops ? o1 : A.nops);
        sp_for_ops<64>(P, 0, o1, lane, [&](const SpPair &p) { sp_rotate_pair(psi, cs, p); });   // psi alone
        sp_for_ops<64>(P, o1, A.nops, lane, [&](const SpPair &p) { sp_tangent_pair(psi, t, cs, dk, p); });   // psi and the tangent
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        for (int i = lane; i < A.m; i += 64) store[(size_t)i * (size_t)A.wpad + (size_t)k] = t[i];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
}

// ---- exact energy Hessian on the compact support (ovqe_energy_hessian, path 1) ------------------------------------------------------------
// All K x K second derivatives of one parameter vector in ONE launch, forward over reverse (the derivation: sv_hessian_host.hpp).  Workgroup
// (one wave) b owns the direction b: it carries psi and the tangent t = d psi / d theta_b forward exactly as k_sparse_metric does, forms
// lambda = H psi and mu = H t in one pass over the restricted Hamiltonian's entries (the LDS atomics of k_sparse_grad's lambda loop,
// doubled), and walks the program backwards on the four vectors: per pair the gradient's weight g and its derivative
//   g' = mu_i psi_j - mu_j psi_i + lambda_i t_j - lambda_j t_i                                 (on the states before un-applying)
// go to w[e] / wd[e] with the pair's sign, the four vectors are rotated back, and an entry of parameter b injects -coeff_e J of the
// un-applied psi and lambda into t and mu.  Below first_op[b] the tangent is exactly zero and is dropped: psi, lambda and mu remain.
// Row b of the raw matrix is sum over the entries of parameter k of 2 coeff_e wd[e]; the workgroup of direction 0 accumulates w as well
// and writes the energy and the gradient.  The program, its table and first_op are the metric's (sv_metric_host.hpp), the entries are built
// on THAT program's compact indices.  The order of the atomic additions is not fixed: the result reproduces to rounding, not to the bit.
// (This kernel keeps its walks spelled out instead of going through sp_for_ops and the Givens helpers above: rewritten on them it
// issued the same vector instructions but ran 3 us slower per launch on H2O (126 -> 129 us; profiles/sparse_walk/README.md).)
template <bool STAGE>
__global__ __launch_bounds__(64) void k_sparse_hessian(SpHessArgs A, const double *__restrict__ theta, const metric::TabEntry *__restrict__ tab,
                                                       const metric::Op *__restrict__ ops, const uint32_t *__restrict__ pairs,
                                                       const int32_t *__restrict__ first_op, const SpEntry *__restrict__ entries,
                                                       double *__restrict__ rows, double *__restrict__ energy, double *__restrict__ grad) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const SpHessLds L = sp_hessian_lds(A, STAGE);
    double *psi = reinterpret_cast<double *>(smem);
    double *t = reinterpret_cast<double *>(smem + L.t);
    double *lam = reinterpret_cast<double *>(smem + L.lam);
    double *mu = reinterpret_cast<double *>(smem + L.mu);
    double2 *cs = reinterpret_cast<double2 *>(smem + L.cs);
    double *dk = reinterpret_cast<double *>(smem + L.dk);
    double *w = reinterpret_cast<double *>(smem + L.w);
    double *wd = reinterpret_cast<double *>(smem + L.wd);
    double *gk = reinterpret_cast<double *>(smem + L.gk);
    metric::Op *lops = reinterpret_cast<metric::Op *>(smem + L.ops);
    uint32_t *lpairs = reinterpret_cast<uint32_t *>(smem + L.pairs);
    const int lane = threadIdx.x;
    if constexpr (STAGE) {
        for (int i = lane; i < A.nops; i += 64) lops[i] = ops[i];
        for (int i = lane; i < A.npairs; i += 64) lpairs[i] = pairs[i];
    }
    const metric::Op *opv = STAGE ? lops : ops;
    const uint32_t *pv = STAGE ? lpairs : pairs;
    for (int b = blockIdx.x; b < A.K; b += gridDim.x) {
        const bool first = b == 0;   // (uniform: this direction's workgroup also answers E and the gradient)
        for (int i = lane; i < A.mpad; i += 64) {
            psi[i] = i == A.hf ? 1.0 : 0.0;
            t[i] = 0.0;
            lam[i] = 0.0;
            mu[i] = 0.0;
        }
        for (int e = lane; e < A.ntab; e += 64) {
            const metric::TabEntry te = tab[e];
            double sn, c;
            sincos(te.phi0 + (te.pidx >= 0 ? te.coeff * theta[te.pidx] : 0.0), &sn, &c);
            cs[e] = make_double2(c, sn);
            dk[e] = te.pidx == b ? te.coeff : 0.0;
            w[e] = 0.0;
            wd[e] = 0.0;
        }
        for (int k = lane; k < A.K; k += 64) gk[k] = 0.0;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        int o1 = first_op[b];
        o1 = __builtin_amdgcn_readfirstlane(o1 < A.nops ? o1 : A.nops);
        // ---- forward, as k_sparse_metric: psi alone, then psi and the tangent
        for (int o = 0; o < o1; ++o) {
            metric::Op op = opv[o];
            op.first = __builtin_amdgcn_readfirstlane(op.first);
            op.npairs = __builtin_amdgcn_readfirstlane(op.npairs);
            op.tab0 = __builtin_amdgcn_readfirstlane(op.tab0);
            for (int pe = lane; pe < op.npairs; pe += 64) {
                const uint32_t pw = pv[op.first + pe];
                const uint32_t ci = pw & 0xfffu, cj = (pw >> 12) & 0xfffu;
                const double2 r = cs[op.tab0 + (int)(pw >> 25)];
                const double sn = (pw & (1u << 24)) ? -r.y : r.y;
                const double u = psi[ci], v = psi[cj];
                psi[ci] = r.x * u + sn * v;
                psi[cj] = r.x * v - sn * u;
            }
            asm volatile("" ::: "memory");   // a wave's DS instructions execute in issue order (see k_sparse_vqe)
        }
        for (int o = o1; o < A.nops; ++o) {
            metric::Op op = opv[o];
            op.first = __builtin_amdgcn_readfirstlane(op.first);
            op.npairs = __builtin_amdgcn_readfirstlane(op.npairs);
            op.tab0 = __builtin_amdgcn_readfirstlane(op.tab0);
            for (int pe = lane; pe < op.npairs; pe += 64) {
                const uint32_t pw = pv[op.first + pe];
                const uint32_t ci = pw & 0xfffu, cj = (pw >> 12) & 0xfffu;
                const int e = op.tab0 + (int)(pw >> 25);
                const double2 r = cs[e];
                const bool neg = (pw & (1u << 24)) != 0u;
                const double sn = neg ? -r.y : r.y;
                const double d = neg ? -dk[e] : dk[e];
                const double u = psi[ci], v = psi[cj], tu = t[ci], tv = t[cj];
                const double u1 = r.x * u + sn * v, v1 = r.x * v - sn * u;
                psi[ci] = u1;
                psi[cj] = v1;
                t[ci] = r.x * tu + sn * tv + d * v1;
                t[cj] = r.x * tv - sn * tu - d * u1;
            }
            asm volatile("" ::: "memory");
        }
        // ---- lambda = H psi and mu = H t in one pass over the entries, E = <psi|lambda>
        double acc = 0.0;
#pragma unroll 2
        for (int e = lane; e < A.nent; e += 64) {
            const SpEntry en = entries[e];
            const uint32_t ci = en.ij & 0xfffu, cj = (en.ij >> 12) & 0xfffu;
            const double ai = psi[ci], aj = psi[cj], ti = t[ci], tj = t[cj];
            acc += en.c * ai * aj;
            if (ci == cj) {
                __hip_atomic_fetch_add(&lam[ci], en.c * ai, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_fetch_add(&mu[ci], en.c * ti, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            } else {   // c = 2 H_ij, the pair counted once
                const double hc = 0.5 * en.c;
                __hip_atomic_fetch_add(&lam[ci], hc * aj, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_fetch_add(&lam[cj], hc * ai, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_fetch_add(&mu[ci], hc * tj, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_fetch_add(&mu[cj], hc * ti, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
        const double etot = wave_sum(acc);
        if (first && lane == 0) energy[0] = etot + A.constant;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        // ---- backward on the four vectors, with the injections and both weights
        for (int o = A.nops - 1; o >= o1; --o) {
            metric::Op op = opv[o];
            op.first = __builtin_amdgcn_readfirstlane(op.first);
            op.npairs = __builtin_amdgcn_readfirstlane(op.npairs);
            op.tab0 = __builtin_amdgcn_readfirstlane(op.tab0);
            for (int pe = lane; pe < op.npairs; pe += 64) {
                const uint32_t pw = pv[op.first + pe];
                const uint32_t ci = pw & 0xfffu, cj = (pw >> 12) & 0xfffu;
                const int e = op.tab0 + (int)(pw >> 25);
                const double2 r = cs[e];
                const bool neg = (pw & (1u << 24)) != 0u;
                const double sn = neg ? -r.y : r.y;
                const double d = neg ? -dk[e] : dk[e];
                const double u1 = psi[ci], v1 = psi[cj], lu = lam[ci], lv = lam[cj];
                const double tu = t[ci], tv = t[cj], mu1 = mu[ci], mv1 = mu[cj];
                const double gd = mu1 * v1 - mv1 * u1 + lu * tv - lv * tu;
                __hip_atomic_fetch_add(&wd[e], neg ? -gd : gd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (first) {
                    const double g = lu * v1 - lv * u1;
                    __hip_atomic_fetch_add(&w[e], neg ? -g : g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
                const double u0 = r.x * u1 - sn * v1, v0 = r.x * v1 + sn * u1;
                const double lu0 = r.x * lu - sn * lv, lv0 = r.x * lv + sn * lu;
                psi[ci] = u0;
                psi[cj] = v0;
                lam[ci] = lu0;
                lam[cj] = lv0;
                t[ci] = r.x * tu - sn * tv - d * v0;
                t[cj] = r.x * tv + sn * tu + d * u0;
                mu[ci] = r.x * mu1 - sn * mv1 - d * lv0;
                mu[cj] = r.x * mv1 + sn * mu1 + d * lu0;
            }
            asm volatile("" ::: "memory");
        }
        for (int o = o1 - 1; o >= 0; --o) {   // the tangent is zero from here down: psi, lambda and mu
            metric::Op op = opv[o];
            op.first = __builtin_amdgcn_readfirstlane(op.first);
            op.npairs = __builtin_amdgcn_readfirstlane(op.npairs);
            op.tab0 = __builtin_amdgcn_readfirstlane(op.tab0);
            for (int pe = lane; pe < op.npairs; pe += 64) {
                const uint32_t pw = pv[op.first + pe];
                const uint32_t ci = pw & 0xfffu, cj = (pw >> 12) & 0xfffu;
                const int e = op.tab0 + (int)(pw >> 25);
                const double2 r = cs[e];
                const bool neg = (pw & (1u << 24)) != 0u;
                const double sn = neg ? -r.y : r.y;
                const double u1 = psi[ci], v1 = psi[cj], lu = lam[ci], lv = lam[cj], mu1 = mu[ci], mv1 = mu[cj];
                const double gd = mu1 * v1 - mv1 * u1;
                __hip_atomic_fetch_add(&wd[e], neg ? -gd : gd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (first) {
                    const double g = lu * v1 - lv * u1;
                    __hip_atomic_fetch_add(&w[e], neg ? -g : g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
                psi[ci] = r.x * u1 - sn * v1;
                psi[cj] = r.x * v1 + sn * u1;
                lam[ci] = r.x * lu - sn * lv;
                lam[cj] = r.x * lv + sn * lu;
                mu[ci] = r.x * mu1 - sn * mv1;
                mu[cj] = r.x * mv1 + sn * mu1;
            }
            asm volatile("" ::: "memory");
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        // ---- row b: sum over the entries of parameter k of 2 coeff_e wd[e]
        for (int e = lane; e < A.ntab; e += 64) {
            const metric::TabEntry te = tab[e];
            if (te.pidx >= 0) __hip_atomic_fetch_add(&gk[te.pidx], 2.0 * te.coeff * wd[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        for (int k = lane; k < A.K; k += 64) rows[(size_t)b * (size_t)A.K + (size_t)k] = gk[k];
        if (first) {   // ... and the gradient, through the same slots
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            for (int k = lane; k < A.K; k += 64) gk[k] = 0.0;
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            for (int e = lane; e < A.ntab; e += 64) {
                const metric::TabEntry te = tab[e];
                if (te.pidx >= 0) __hip_atomic_fetch_add(&gk[te.pidx], 2.0 * te.coeff * w[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            for (int k = lane; k < A.K; k += 64) grad[k] = gk[k];
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
}

}  // namespace ovqe
