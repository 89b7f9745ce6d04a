// sv_pool.hpp — the ADAPT pool screen ACROSS two shards of the partitioned register: every operator of a pass from one LDS tile.
//
// The pool form of sv_cross.hpp's tile-cover machinery (plan: sv_pool_host.hpp).  A pass has a set S of M index bits inside the chunk
// and a displacement d_out outside S.  The workgroup of ket tile t stages that tile of psi (from the received partner chunk, or from
// the own shard for d = 0) in LDS, every thread holds the amplitudes of the BRA (sigma, resident on this rank) at tile t ^ d_out in
// registers, and every pool ENTRY of the pass — (operator slot k, x mask inside S, terms t0..t1) — is evaluated from that one staging:
//
//   v_k += sum_i conj(sigma_i) [sum_t c_t (-1)^{|j & z_t|}] psi_j,   j = i ^ x.
//
// Unlike k_tile_cross<DOT> the product with the bra is taken PER ENTRY and lands in a per-operator accumulator: entries with the same
// x that belong to different operators never merge.  A pass moves 32 B per amplitude (16 B on real shards) whatever its entries.
//
// Reductions, all in a fixed order (no floating-point atomics; bit-identical from run to run): lanes of a wave by shuffles, the waves
// of a workgroup through an LDS row per wave, summed wave 0 .. NT/64 - 1 by the thread that owns the entry's run of equal slots in
// the staged chunk, which adds the sum to ITS workgroup's row of the partials: partials[blockIdx.x * n_slots + k].  A workgroup
// walks its tiles (blockIdx.x, + gridDim.x, ...) and its chunks in order, barriers in between; launches on one stream are ordered.
// The grid is at most POOL_ROWS workgroups, so the partials are POOL_ROWS x n_slots double2 whatever the shard; k_pool_finish sums
// the rows 0 .. POOL_ROWS - 1 per operator and clears them.
#pragma once
#include "sv_pool_host.hpp"
#include "sv_tile.hpp"

namespace ovqe {

using pool::PoolEntry;

// dynamic LDS of k_tile_pool / k_tile_pool_real, one definition for kernel and host: [tile][terms][entries][one row per wave]
struct TilePoolLds { size_t terms, entries, wacc, bytes; };   // the tile is at 0
template <int M>
__host__ __device__ constexpr TilePoolLds tile_pool_lds(size_t amp_bytes, int waves) {
    const size_t terms = amp_bytes << M;
    const size_t entries = terms + pool::POOL_TERM_CAP * sizeof(ExTermLds);
    const size_t wacc = entries + pool::POOL_ENTRY_CAP * sizeof(PoolEntry);
    return {terms, entries, wacc, wacc + (size_t)waves * pool::POOL_ENTRY_CAP * sizeof(double2)};
}

// the flush of one staged chunk: the head of every run of equal slots sums its entries over the waves and adds to the row
__device__ __forceinline__ void pool_flush(const PoolEntry *le, const double2 *wacc, int ng, int waves, double2 *__restrict__ row) {
    for (int g = (int)threadIdx.x; g < ng; g += (int)blockDim.x) {
        const PoolEntry en = le[g];
        if (en.run <= 0) continue;
        double2 s = make_double2(0.0, 0.0);
        for (int r = g; r < g + en.run; ++r)
            for (int w = 0; w < waves; ++w) {
                const double2 v = wacc[w * pool::POOL_ENTRY_CAP + r];
                s.x += v.x;
                s.y += v.y;
            }
        const double2 o = row[en.slot];
        row[en.slot] = make_double2(o.x + s.x, o.y + s.y);
    }
}

template <int M, int NT, bool NTL>
__global__ __launch_bounds__(NT) void k_tile_pool(const amp_t *__restrict__ ket, const amp_t *__restrict__ bra, uint64_t ket_gbase,
                                                  uint64_t chunk_off, TilePass ps, uint32_t ntiles, const ExChunkT *__restrict__ chunks,
                                                  const PoolEntry *__restrict__ entries, const ExTermT *__restrict__ terms,
                                                  double2 *__restrict__ partials, int n_slots) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr uint32_t NEL = 1u << M;
    constexpr int TRIPS = NEL / NT;
    constexpr int WAVES = NT / 64;
    double2 *tile = reinterpret_cast<double2 *>(smem);
    constexpr TilePoolLds L = tile_pool_lds<M>(sizeof(double2), WAVES);
    ExTermLds *lt = reinterpret_cast<ExTermLds *>(smem + L.terms);
    PoolEntry *le = reinterpret_cast<PoolEntry *>(smem + L.entries);
    double2 *wacc = reinterpret_cast<double2 *>(smem + L.wacc);
    const v2d *p = reinterpret_cast<const v2d *>(ket);
    const v2d *q = reinterpret_cast<const v2d *>(bra);
    double2 *row = partials + (size_t)blockIdx.x * (size_t)n_slots;
    const uint64_t glow = spread_bits(threadIdx.x, ps.mask_lo);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

    for (uint32_t tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
        uint64_t tb = tl;   // the ket tile: its number spread over the chunk's index bits outside S
        for (uint64_t mk = ps.smask; mk; mk &= mk - 1ull) tb = insert_zero(tb, __ffsll((long long)mk) - 1);
        const uint64_t gbase = ket_gbase | tb;
        const uint64_t ob = (chunk_off | tb) ^ ps.d_out;   // the bra tile, local index space of the shard
        bool any = false;
        {
            v2d reg[TRIPS];
#pragma unroll
            for (int j = 0; j < TRIPS; ++j) {
                const uint64_t hi = spread_bits((uint32_t)j, ps.mask_hi);
                reg[j] = NTL ? __builtin_nontemporal_load(&p[tb | glow | hi]) : p[tb | glow | hi];
            }
#pragma unroll
            for (int j = 0; j < TRIPS; ++j) {
                tile[tile_swz_v(threadIdx.x + j * NT)] = make_double2(reg[j].x, reg[j].y);
                any |= reg[j].x != 0.0 || reg[j].y != 0.0;
            }
        }
        // a ket tile of zeros contributes nothing (an ADAPT state lives on a particle-number sector: most tiles of the register)
        if (!__syncthreads_or(any)) continue;
        v2d b[TRIPS];
#pragma unroll
        for (int j = 0; j < TRIPS; ++j) {
            const uint64_t g = ob | glow | spread_bits((uint32_t)j, ps.mask_hi);
            b[j] = NTL ? __builtin_nontemporal_load(&q[g]) : q[g];
        }
        for (int ch = ps.a0; ch < ps.a1; ++ch) {
            const ExChunkT ck = chunks[ch];
            __syncthreads();   // (the previous chunk's flush has read the tables and the wave rows)
            for (int t = ck.t0 + (int)threadIdx.x; t < ck.t1; t += NT) {
                const ExTermT et = terms[t];
                const bool neg = parity64(gbase & et.zout);
                ExTermLds l;
                l.cr = neg ? -et.cr : et.cr;
                l.ci = neg ? -et.ci : et.ci;
                l.zin = et.zin;
                l.pad = 0;
                lt[t - ck.t0] = l;
            }
            for (int g = ck.g0 + (int)threadIdx.x; g < ck.g1; g += NT) le[g - ck.g0] = entries[g];
            __syncthreads();
            const int ng = ck.g1 - ck.g0;
            for (int g = 0; g < ng; ++g) {
                const PoolEntry en = le[g];
                const uint32_t xl = __builtin_amdgcn_readfirstlane(en.x);
                const int t0 = __builtin_amdgcn_readfirstlane(en.t0) - ck.t0, t1 = __builtin_amdgcn_readfirstlane(en.t1) - ck.t0;
                uint32_t je[TRIPS];
                double dr[TRIPS], di[TRIPS];
#pragma unroll
                for (int j = 0; j < TRIPS; ++j) {
                    je[j] = (threadIdx.x + j * NT) ^ xl;   // the ket's tile-local index: the sign of a term is read off IT
                    dr[j] = 0.0;
                    di[j] = 0.0;
                }
                for (int t = t0; t < t1; ++t) {
                    const ExTermLds l = lt[t];
#pragma unroll
                    for (int j = 0; j < TRIPS; ++j) {
                        const double sg = parity_sign(je[j] & l.zin);
                        dr[j] = fma(l.cr, sg, dr[j]);
                        di[j] = fma(l.ci, sg, di[j]);
                    }
                }
                double2 part = make_double2(0.0, 0.0);   // conj(bra_i) D(j) ket_j
#pragma unroll
                for (int j = 0; j < TRIPS; ++j) {
                    const double2 k = tile[tile_swz_v(je[j])];
                    const double sx = dr[j] * k.x - di[j] * k.y, sy = dr[j] * k.y + di[j] * k.x;
                    part.x += b[j].x * sx + b[j].y * sy;
                    part.y += b[j].x * sy - b[j].y * sx;
                }
                part.x = wave_sum(part.x);
                part.y = wave_sum(part.y);
                if (lane == 0) wacc[wave * pool::POOL_ENTRY_CAP + g] = part;
            }
            __syncthreads();
            pool_flush(le, wacc, ng, WAVES, row);
        }
        __syncthreads();   // (the flush is done before the next tile's chunks restage; the row's stores precede its next reads)
    }
}

// REAL amplitudes (2^n doubles): psi and sigma real, the pair-index convention of k_tile_cross_real (the 16-byte element is a PAIR of
// amplitudes, the pass's masks live in the index space of the pairs, the tile holds 2^M doubles).  BOTH parts of v_k are kept: terms
// whose folded coefficient c i^ny is real give Re v_k, terms whose folded coefficient is imaginary give Im v_k (a qubit-pool string
// with an odd number of Y is purely imaginary between real vectors; its gradient is 2 |v_k|) — nothing is dropped as the <H> cover does.
template <int M, int NT, bool NTL>
__global__ __launch_bounds__(NT) void k_tile_pool_real(const double *__restrict__ ket, const double *__restrict__ bra, uint64_t ket_gbase,
                                                       uint64_t chunk_off, TilePass ps, uint32_t ntiles,
                                                       const ExChunkT *__restrict__ chunks, const PoolEntry *__restrict__ entries,
                                                       const ExTermT *__restrict__ terms, double2 *__restrict__ partials, int n_slots) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr uint32_t NEL = 1u << M;
    constexpr uint32_t NELV = NEL / 2;
    constexpr int TRIPS = NELV / NT;
    constexpr int WAVES = NT / 64;
    double *tile = reinterpret_cast<double *>(smem);
    double2 *tilev = reinterpret_cast<double2 *>(smem);
    constexpr TilePoolLds L = tile_pool_lds<M>(sizeof(double), WAVES);
    ExTermLds *lt = reinterpret_cast<ExTermLds *>(smem + L.terms);
    PoolEntry *le = reinterpret_cast<PoolEntry *>(smem + L.entries);
    double2 *wacc = reinterpret_cast<double2 *>(smem + L.wacc);
    const v2d *p = reinterpret_cast<const v2d *>(ket);
    const v2d *q = reinterpret_cast<const v2d *>(bra);
    double2 *row = partials + (size_t)blockIdx.x * (size_t)n_slots;
    const uint64_t glow = spread_bits(threadIdx.x, ps.mask_lo);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

    for (uint32_t tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
        uint64_t tb = tl;   // pair-index space
        for (uint64_t mk = ps.smask; mk; mk &= mk - 1ull) tb = insert_zero(tb, __ffsll((long long)mk) - 1);
        const uint64_t gbase = ket_gbase | (tb << 1);
        const uint64_t ob = ((chunk_off >> 1) | tb) ^ (ps.d_out >> 1);
        bool any = false;
        {
            v2d reg[TRIPS];
#pragma unroll
            for (int j = 0; j < TRIPS; ++j) {
                const uint64_t hi = spread_bits((uint32_t)j, ps.mask_hi);
                reg[j] = NTL ? __builtin_nontemporal_load(&p[tb | glow | hi]) : p[tb | glow | hi];
            }
#pragma unroll
            for (int j = 0; j < TRIPS; ++j) {
                tilev[tile_swz_v(threadIdx.x + j * NT)] = make_double2(reg[j].x, reg[j].y);
                any |= reg[j].x != 0.0 || reg[j].y != 0.0;
            }
        }
        if (!__syncthreads_or(any)) continue;
        v2d b[TRIPS];
#pragma unroll
        for (int j = 0; j < TRIPS; ++j) {
            const uint64_t g = ob | glow | spread_bits((uint32_t)j, ps.mask_hi);
            b[j] = NTL ? __builtin_nontemporal_load(&q[g]) : q[g];
        }
        for (int ch = ps.a0; ch < ps.a1; ++ch) {
            const ExChunkT ck = chunks[ch];
            __syncthreads();
            for (int t = ck.t0 + (int)threadIdx.x; t < ck.t1; t += NT) {
                const ExTermT et = terms[t];
                const bool neg = parity64(gbase & et.zout);
                ExTermLds l;
                l.cr = neg ? -et.cr : et.cr;
                l.ci = neg ? -et.ci : et.ci;
                l.zin = et.zin;
                l.pad = 0;
                lt[t - ck.t0] = l;
            }
            for (int g = ck.g0 + (int)threadIdx.x; g < ck.g1; g += NT) le[g - ck.g0] = entries[g];
            __syncthreads();
            const int ng = ck.g1 - ck.g0;
            for (int g = 0; g < ng; ++g) {
                const PoolEntry en = le[g];
                const uint32_t xl = __builtin_amdgcn_readfirstlane(en.x);
                const int t0 = __builtin_amdgcn_readfirstlane(en.t0) - ck.t0, t1 = __builtin_amdgcn_readfirstlane(en.t1) - ck.t0;
                uint32_t je0[TRIPS], je1[TRIPS];
                double dr0[TRIPS], dr1[TRIPS], di0[TRIPS], di1[TRIPS];
#pragma unroll
                for (int j = 0; j < TRIPS; ++j) {
                    const uint32_t e = (threadIdx.x + j * NT) << 1;
                    je0[j] = e ^ xl;
                    je1[j] = (e | 1u) ^ xl;
                    dr0[j] = dr1[j] = di0[j] = di1[j] = 0.0;
                }
                for (int t = t0; t < t1; ++t) {
                    const ExTermLds l = lt[t];
#pragma unroll
                    for (int j = 0; j < TRIPS; ++j) {
                        const double s0 = parity_sign(je0[j] & l.zin), s1 = parity_sign(je1[j] & l.zin);
                        dr0[j] = fma(l.cr, s0, dr0[j]);
                        di0[j] = fma(l.ci, s0, di0[j]);
                        dr1[j] = fma(l.cr, s1, dr1[j]);
                        di1[j] = fma(l.ci, s1, di1[j]);
                    }
                }
                double2 part = make_double2(0.0, 0.0);
#pragma unroll
                for (int j = 0; j < TRIPS; ++j) {
                    const double w0 = b[j].x * tile[tile_swz<true>(je0[j])], w1 = b[j].y * tile[tile_swz<true>(je1[j])];
                    part.x += dr0[j] * w0 + dr1[j] * w1;
                    part.y += di0[j] * w0 + di1[j] * w1;
                }
                part.x = wave_sum(part.x);
                part.y = wave_sum(part.y);
                if (lane == 0) wacc[wave * pool::POOL_ENTRY_CAP + g] = part;
            }
            __syncthreads();
            pool_flush(le, wacc, ng, WAVES, row);
        }
        __syncthreads();
    }
}

// Chunks below the tile sizes (the CPU-sized tests): the streaming form.  Entries [e0, e1) share the part of their x mask above the
// chunk bits (one launch per class); `bra` is the class's bra chunk, PoolEntry::x the x mask on the chunk bits, ExTermT::zout the
// full z mask (the sign is read off the ket's GLOBAL index ket_gbase | j).  A workgroup strides over the chunk once per entry and
// adds the entry's block sum to its row: POOL_SMALL_ROWS rows.
template <bool REAL>
__global__ __launch_bounds__(256) void k_pool_small(const void *__restrict__ ket_, const void *__restrict__ bra_, uint64_t csize,
                                                    uint64_t ket_gbase, const PoolEntry *__restrict__ entries, int e0, int e1,
                                                    const ExTermT *__restrict__ terms, double2 *__restrict__ partials, int n_slots) {
    __shared__ double2 red[4];
    typedef typename Amp<REAL>::T amp;
    const amp *ket = reinterpret_cast<const amp *>(ket_), *bra = reinterpret_cast<const amp *>(bra_);
    double2 *row = partials + (size_t)blockIdx.x * (size_t)n_slots;
    for (int e = e0; e < e1; ++e) {
        const PoolEntry en = entries[e];
        double2 part = make_double2(0.0, 0.0);
        for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < csize; i += (uint64_t)gridDim.x * 256u) {
            const uint64_t j = i ^ en.x;
            const uint64_t gj = ket_gbase | j;
            double dr = 0.0, di = 0.0;
            for (int t = en.t0; t < en.t1; ++t) {
                const ExTermT pt = terms[t];
                const double sg = parity_sign64(gj & pt.zout);
                dr = fma(pt.cr, sg, dr);
                di = fma(pt.ci, sg, di);
            }
            if constexpr (REAL) {
                const double w = bra[i] * ket[j];
                part.x += dr * w;
                part.y += di * w;
            } else {
                const amp k = ket[j], bb = bra[i];
                const double sx = dr * k.x - di * k.y, sy = dr * k.y + di * k.x;
                part.x += bb.x * sx + bb.y * sy;
                part.y += bb.x * sy - bb.y * sx;
            }
        }
        const double2 t = block_sum<256>(part, red);
        if (threadIdx.x == 0) {
            const double2 o = row[en.slot];
            row[en.slot] = make_double2(o.x + t.x, o.y + t.y);
        }
    }
}

// v_k = the rows 0 .. rows - 1 of operator k in that order; the rows are cleared for the next screen
__global__ __launch_bounds__(256) void k_pool_finish(double2 *__restrict__ partials, int rows, int n_slots, double2 *__restrict__ out) {
    const int k = (int)(blockIdx.x * 256u + threadIdx.x);
    if (k >= n_slots) return;
    double2 s = make_double2(0.0, 0.0);
    for (int r = 0; r < rows; ++r) {
        const double2 v = partials[(size_t)r * (size_t)n_slots + k];
        s.x += v.x;
        s.y += v.y;
        partials[(size_t)r * (size_t)n_slots + k] = make_double2(0.0, 0.0);
    }
    out[k] = s;
}

}  // namespace ovqe
