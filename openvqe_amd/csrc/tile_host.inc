// tile_host.inc — the LDS-tiled paths of the full register: planner and launches of the tiled <H> (cover sets, entries, the Walsh-Hadamard
// diagonal group), the compact cover, and the multi-op tile sweeps (kernels: sv_tile.hpp).  Included by ovqe_sv.hip inside its anonymous namespace.

// ---- tiled expectation (sv_tile.hpp) -----------------------------------------------------------------------
// Greedy cover of the x-groups by tile bit sets: a set starts from the mandatory low bits and grows by grow_tile_set()
// (sv_cover_host.hpp) over the still-uncovered groups.
static int achunks_g0(const std::vector<ExChunkT> &a, int a0, const ExChunkT &cur) { return a0 < (int)a.size() ? a[a0].g0 : cur.g0; }
static int achunks_t0(const std::vector<ExChunkT> &a, int a0, const ExChunkT &cur) { return a0 < (int)a.size() ? a[a0].t0 : cur.t0; }

// the trip part of an entry's pair index, for tile_entry_pairs (sv_tile.hpp ExEntryT::pb / tsign): deposit of the trip counter's bits
// over the positions outside x, swizzled byte offsets, the terms' parities on the partner index
inline uint32_t host_deposit(uint32_t k, uint32_t fixmask) {
    for (uint32_t m = fixmask; m; m &= m - 1u) {
        const uint32_t low = (m & (0u - m)) - 1u;
        k = ((k & ~low) << 1) | (k & low);
    }
    return k;
}
inline uint32_t host_tile_swz(uint32_t e, bool real) { return real ? e ^ (((e >> 4) & 7u) << 1) : e ^ ((e >> 3) & 7u); }
void fill_entry_basis(ExEntryT &en, const std::vector<ExTermT> &tterms, bool real, int M) {
    const uint32_t nel = 1u << M, ab = real ? 8u : 16u;
    const uint32_t xf = en.pad ? (uint32_t)en.pad : en.x;
    const uint32_t iu0 = (host_deposit((uint32_t)en.k0, en.x) | en.ibits) & (nel - 1u);
    uint32_t d[4];
    for (int b = 0; b < 4; ++b) d[b] = host_deposit(64u << b, en.x) & (nel - 1u);
    en.tsign = 0;
    const int nt = std::min(2, en.t1 - en.t0);
    for (uint32_t t = 0; t < 16u; ++t) {
        uint32_t iu = iu0;                                  // trip t's share of the pair index: trip 0's XOR one basis value per set bit of t
        for (int b = 0; b < 4; ++b)
            if ((t >> b) & 1u) iu ^= d[b];
        en.ph[t] = host_tile_swz(iu, real) * ab;
        for (int j = 0; j < nt; ++j) {
            const uint32_t zin = tterms[(size_t)en.t0 + (j == 0 ? 0 : (en.t1 - en.t0 - 1))].zin;   // (the kernel takes the first and the LAST term)
            en.tsign |= ((uint32_t)__builtin_popcount((iu ^ xf) & zin) & 1u) << (16 * j + t);
        }
    }
}

int build_ham_tiles(ovqe_handle h, HamDev &H, bool real) {
    const int M = tile_bits(h, real), L = HAM_TILE_LOW;
    H.tile_bits = M;
    H.tile_low = L;
    H.tile_real = real;
    H.tsweeps.clear();
    H.tsweep_terms.clear();
    H.h_achunks.clear();
    H.cover_id++;
    H.n_rest = 0;
    H.tile_work = 0;
    H.diag_sweep = -1;
    H.diag_nu = 0;
    const bool tiled = tile_ok(h, real) && H.groups.size() >= 3;
    if (!tiled) return OVQE_OK;
    const int G = (int)H.groups.size();
    const uint64_t lowbits = (1ull << L) - 1ull;
    std::vector<char> covered(G, 0);
    std::vector<ExChunkT> chunks;
    std::vector<ExEntryT> tgroups;
    std::map<std::pair<uint64_t, uint64_t>, std::pair<double, double>> merged;
    std::vector<ExTermT> tterms;
    std::vector<ExFlatT> tflats;
    std::vector<ExItemT> titems;
    std::vector<ExChunkT> achunks;
    std::vector<ExAGroupT> agroups;
    std::vector<ExTermT> aterms;
    std::vector<HGroup> rest;
    int remaining = 0;
    for (int g = 0; g < G; ++g) {
        if (__builtin_popcountll(H.groups[g].x | lowbits) > M) {
            covered[g] = 2;
            rest.push_back(H.groups[g]);
        } else {
            ++remaining;
        }
    }
    while (remaining > 0) {
        std::vector<uint64_t> uncovered;
        for (int g = 0; g < G; ++g)
            if (!covered[g]) uncovered.push_back(H.groups[g].x);
        const uint64_t S = grow_tile_set(uncovered, lowbits, M, h->n_local);
        ExSweep sw = {};
        sw.smask = real ? S >> 1 : S;  // real state: masks in the index space of amplitude pairs (sv_tile.hpp)
        std::tie(sw.mask_lo, sw.mask_hi) = thread_trip_masks(sw.smask, TILE_EXPECT_LOG_NT);
        sw.c0 = (int32_t)chunks.size();
        sw.i0 = (int32_t)titems.size();
        ExChunkT ck = open_chunk(tgroups.size(), tterms.size());
        int took = 0;
        sw.a0 = (int32_t)achunks.size();
        ExChunkT ak = open_chunk(agroups.size(), aterms.size());
        for (int g = 0; g < G; ++g) {
            if (covered[g] || (H.groups[g].x & ~S)) continue;
            covered[g] = 1;
            --remaining;
            ++took;
            const HGroup &gr = H.groups[g];
            if (gr.x == 0) H.diag_sweep = (int)H.tsweeps.size();   // (this sweep; pushed below)
            const uint32_t xl = extract_bits(gr.x, S);
            {   // operator-application form (k_tile_apply; sparse tiles of k_tile_expect): the group's raw terms, split
                // when they exceed a chunk.  Real state: strings with an imaginary folded coefficient (odd number of
                // Y) have <P> = 0 and are left out.
                std::vector<int> keep;
                for (int t = gr.t0; t < gr.t1; ++t)
                    if (!(real && H.terms[t].ci != 0.0)) keep.push_back(t);
                // a group enters in pieces of at most TILE_APPLY_TERMS terms (D_g is a sum over its terms, so the pieces
                // are independent work units): one wave serves a piece, and the diagonal group with its hundreds of
                // Z strings no longer keeps a single wave busy while the others idle
                for (size_t k0 = 0; k0 < keep.size(); k0 += TILE_APPLY_TERMS) {
                    const size_t k1 = std::min(keep.size(), k0 + TILE_APPLY_TERMS);
                    stage_piece(achunks, ak, agroups.size(), aterms.size(), k1 - k0, TILE_TERM_CAP, TILE_APPLY_GROUPS);
                    ExAGroupT ag = {xl, (int32_t)aterms.size(), 0, 0};
                    for (size_t k = k0; k < k1; ++k) aterms.push_back(tile_term(H.terms[keep[k]], S));
                    ag.t1 = (int32_t)aterms.size();
                    ag.pad = 1;   // bit 0: every folded coefficient of the piece is real (a real-symmetric H: all of them)
                    for (int32_t t = ag.t0; t < ag.t1; ++t)
                        if (aterms[t].ci != 0.0) ag.pad = 0;
                    agroups.push_back(ag);
                }
            }
            const int w = __builtin_popcount(xl);
            int xpos[16], np = 0;
            for (uint32_t mk2 = xl; mk2; mk2 &= mk2 - 1u) xpos[np++] = __builtin_ctz(mk2);
            // UNSPLIT entries (round 5): a group of one or two raw terms on a complex state — no pattern of its x bits cancels, so
            // cutting it into 2^(w-1) pattern entries only multiplies the per-entry set-up (a quarter of the kernel's instructions at
            // w = 4: 25 per pair).  Its 2^(M-1) pairs (pivot bit of i clear) are walked in pieces of 512 with the x part of z left in
            // the terms' masks; en.x = the pivot bit alone (what the index walk skips), en.pad = the mask that leads to the partner.
            if (!real && w >= 2 && gr.t1 - gr.t0 <= 2 && M - 1 >= 9) {
                stage_piece(chunks, ck, tgroups.size(), tterms.size(), (size_t)(gr.t1 - gr.t0), TILE_TERM_CAP);
                const int32_t t0 = (int32_t)tterms.size();
                bool real_only = true;
                for (int t = gr.t0; t < gr.t1; ++t) {
                    if (H.terms[t].ci != 0.0) real_only = false;
                    tterms.push_back(tile_term(H.terms[t], S));
                }
                const int npairs = 1 << (M - 1), piece = std::min(npairs, TILE_UNSPLIT_PAIRS);
                for (int k0 = 0; k0 < npairs; k0 += piece) {
                    ExEntryT en = {};
                    en.x = 1u << xpos[w - 1];
                    en.ibits = 0;
                    en.t0 = t0;
                    en.t1 = (int32_t)tterms.size();
                    en.k0 = k0;
                    en.nk = piece;
                    en.real_only = real_only ? 1 : 0;
                    en.pad = (int32_t)xl;
                    fill_entry_basis(en, tterms, real, M);
                    tgroups.push_back(en);
                }
                continue;
            }
            const uint32_t npat = w ? (1u << (w - 1)) : 1u;
            for (uint32_t e = 0; e < npat; ++e) {
                uint32_t ibits = 0;
                for (int f = 0; f + 1 < w; ++f)
                    if ((e >> f) & 1u) ibits |= 1u << xpos[f];
                const uint32_t jx = ibits ^ xl;  // the partner's bits on the x positions
                // merge the terms that agree outside x: key = (z on the tile without x, z outside the tile)
                merged.clear();
                for (int t = gr.t0; t < gr.t1; ++t) {
                    const HTerm &ht = H.terms[t];
                    if (real && ht.ci != 0.0) continue;  // imaginary folded coefficient: <P> = 0 on a real state
                    const uint32_t zin = extract_bits(ht.z, S);
                    const double sg = (__builtin_popcount(jx & zin) & 1) ? -1.0 : 1.0;
                    auto &slot = merged[std::make_pair((uint64_t)(zin & ~xl), ht.z & ~S)];
                    slot.first += sg * ht.cr;
                    slot.second += sg * ht.ci;
                }
                std::vector<ExTermT> mt;
                bool real_only = true;
                for (const auto &kv : merged) {
                    if (kv.second.first == 0.0 && kv.second.second == 0.0) continue;  // exact cancellation
                    ExTermT et = {};
                    et.zin = (uint32_t)kv.first.first;
                    et.zout = kv.first.second;
                    et.cr = kv.second.first;
                    et.ci = kv.second.second;
                    if (et.ci != 0.0) real_only = false;
                    mt.push_back(et);
                }
                if (mt.empty()) continue;
                const int nk_total = 1 << (M - w);
                // (round 6: the float64 shards of the partitioned register are DENSE real states of 25+ qubits: per-wave entries there too —
                // 31 qubits, 1000-term <H>: 1.09 s with items, 0.94 s with entries, tools/exp_real_shard.py)
                if (mt.size() <= 2 && nk_total >= 2 && (h->opt_tile_flat == 1 || (h->opt_tile_flat == 2 && real && h->n_local < 25))) {  // one lane per TILE_ITEM_PAIRS pairs (sv_tile.hpp)
                    ExFlatT fe = {};
                    fe.x = xl;
                    fe.ibits = ibits;
                    fe.zin0 = mt[0].zin;
                    fe.zout0 = mt[0].zout;
                    fe.c0r = mt[0].cr;
                    fe.c0i = mt[0].ci;
                    if (mt.size() == 2) {
                        fe.zin1 = mt[1].zin;
                        fe.zout1 = mt[1].zout;
                        fe.c1r = mt[1].cr;
                        fe.c1i = mt[1].ci;
                    }
                    for (int k0 = 0; k0 < nk_total; k0 += TILE_ITEM_PAIRS) {
                        uint32_t istart = (uint32_t)k0;  // deposit k0 over the positions outside x, ascending
                        for (int f = 0; f < w; ++f) {
                            const uint32_t low = (1u << xpos[f]) - 1u;
                            istart = ((istart & ~low) << 1) | (istart & low);
                        }
                        titems.push_back(ExItemT{(uint32_t)tflats.size(), istart | ibits,
                                                 (uint32_t)std::min(TILE_ITEM_PAIRS, nk_total - k0), 0u});
                    }
                    tflats.push_back(fe);
                    H.tile_work += (int64_t)nk_total * (int64_t)mt.size();
                    continue;
                }
                for (size_t m0 = 0; m0 < mt.size(); m0 += TILE_TERM_CAP) {  // oversized lists are split (linear)
                    const size_t m1 = std::min(mt.size(), m0 + TILE_TERM_CAP);
                    stage_piece(chunks, ck, tgroups.size(), tterms.size(), m1 - m0, TILE_TERM_CAP);
                    const int32_t t0 = (int32_t)tterms.size();
                    tterms.insert(tterms.end(), mt.begin() + m0, mt.begin() + m1);
                    for (int k0 = 0; k0 < nk_total; k0 += TILE_ENTRY_PAIRS) {
                        ExEntryT en = {};
                        en.x = xl;
                        en.ibits = ibits;
                        en.t0 = t0;
                        en.t1 = (int32_t)tterms.size();
                        en.k0 = k0;
                        en.nk = std::min(TILE_ENTRY_PAIRS, nk_total - k0);
                        en.real_only = real_only ? 1 : 0;
                        if (en.t1 - en.t0 <= 2) fill_entry_basis(en, tterms, real, M);
                        tgroups.push_back(en);
                    }
                }
            }
        }
        close_chunk(chunks, ck, tgroups.size(), tterms.size());
        sw.c1 = (int32_t)chunks.size();
        sw.i1 = (int32_t)titems.size();
        close_chunk(achunks, ak, agroups.size(), aterms.size());
        sw.a1 = (int32_t)achunks.size();
        if (took == 0) return fail(h, OVQE_ERR_INVALID, "internal: tile cover made no progress");
        if (std::getenv("OVQE_DEBUG_COVER"))
            std::fprintf(stderr, "cover sweep %zu: S=%llx groups=%d pieces=%d apply_terms=%d entries=%d items=%d\n",
                         H.tsweeps.size(), (unsigned long long)S, took, (int)agroups.size() - achunks_g0(achunks, sw.a0, ak),
                         (int)aterms.size() - achunks_t0(achunks, sw.a0, ak), (int)tgroups.size() - (int)(sw.c0 < (int)chunks.size() ? chunks[sw.c0].g0 : ck.g0),
                         (int)titems.size() - sw.i0);
        H.tsweeps.push_back(sw);
        H.tsweep_terms.push_back((int)aterms.size() - achunks_t0(achunks, sw.a0, ak));
    }
    H.n_rest = (int)rest.size();
    // the diagonal group in Walsh-Hadamard form (k_tile_diag): contiguous tiles of 2^12 amplitudes, the terms grouped by their z mask
    // on the tile bits (ascending mask, the group's term order inside: a fixed summation order)
    if (H.diag_sweep >= 0 && h->n_local >= 25) {
        const HGroup *dg = nullptr;
        for (const HGroup &g : H.groups)
            if (g.x == 0) dg = &g;
        constexpr int DM = 12;
        if (dg && dg->t1 - dg->t0 >= 12) {
            std::map<uint32_t, std::vector<DiagTermT>> by_zin;
            for (int t = dg->t0; t < dg->t1; ++t)
                by_zin[(uint32_t)(H.terms[t].z & ((1ull << DM) - 1ull))].push_back(DiagTermT{H.terms[t].z >> DM << DM, H.terms[t].cr});
            std::vector<uint32_t> uz;
            std::vector<int32_t> uo = {0};
            std::vector<DiagTermT> dt;
            for (const auto &kv : by_zin) {
                uz.push_back(kv.first);
                dt.insert(dt.end(), kv.second.begin(), kv.second.end());
                uo.push_back((int32_t)dt.size());
            }
            int rc = upload(h, H.d_dzin, uz.data(), uz.size() * sizeof(uint32_t));
            if (!rc) rc = upload(h, H.d_doff, uo.data(), uo.size() * sizeof(int32_t));
            if (!rc) rc = upload(h, H.d_dterms, dt.data(), dt.size() * sizeof(DiagTermT));
            if (rc) return rc;
            H.diag_nu = (int)uz.size();
            H.diag_bits = DM;
        }
    }
    for (const ExEntryT &en : tgroups) H.tile_work += (int64_t)en.nk * (en.t1 - en.t0);
    H.tile_entries = (int64_t)(tgroups.size() + tflats.size());
    H.tile_terms = (int64_t)tterms.size();
    int rc = upload(h, H.d_tchunks, chunks.data(), chunks.size() * sizeof(ExChunkT));
    if (rc) return rc;
    rc = upload(h, H.d_tgroups, tgroups.data(), tgroups.size() * sizeof(ExEntryT));
    if (rc) return rc;
    rc = upload(h, H.d_tterms, tterms.data(), tterms.size() * sizeof(ExTermT));
    if (rc) return rc;
    rc = upload(h, H.d_tflats, tflats.data(), tflats.size() * sizeof(ExFlatT));
    if (rc) return rc;
    rc = upload(h, H.d_titems, titems.data(), titems.size() * sizeof(ExItemT));
    if (rc) return rc;
    H.h_achunks = achunks;
    rc = upload(h, H.d_achunks, achunks.data(), achunks.size() * sizeof(ExChunkT));
    if (!rc) rc = upload(h, H.d_agroups, agroups.data(), agroups.size() * sizeof(ExAGroupT));
    if (!rc) rc = upload(h, H.d_aterms, aterms.data(), aterms.size() * sizeof(ExTermT));
    if (rc) return rc;
    return upload(h, H.d_rest, rest.data(), rest.size() * sizeof(HGroup));
}

inline int expect_ysplit(ovqe_handle h, int M) {  // workgroups per tile: fill the chip when there are few tiles
    const uint64_t tiles = h->namps >> M;
    int y = 1;
    while (y < 8 && tiles * y < 1024) y *= 2;
    return y;
}

// dense_only: the caller knows that no tile of this state is sparse (census of the evaluation's first sweep, run_expectation_tiled):
// the staging area of the sparse-tile path and the tile's non-zero list (38 KB beside a 64-KB tile: ONE workgroup per CU) are left
// out of the launch, and two workgroups share a CU — one loads its tile while the other computes
template <int M, bool REAL>
int launch_tile_expect(ovqe_handle h, const HamDev &H, const ExSweep &sw, double2 *partials, int accumulate,
                       hipStream_t stream, bool dense_only = false, int *census = nullptr, bool skip_diag = false) {
    constexpr int NT = 1 << TILE_EXPECT_LOG_NT;
    static_assert(TILE_SPARSE_TERMS >= 2 * TILE_TERM_CAP && TILE_SPARSE_GROUPS >= 2 * TILE_APPLY_GROUPS, "two host chunks per pass");
    constexpr size_t smem_full = tile_expect_lds<M, NT, REAL>(false).bytes, smem_dense = tile_expect_lds<M, NT, REAL>(true).bytes;
    const size_t smem = dense_only ? smem_dense : smem_full;
    const dim3 grid((unsigned)(h->namps >> M), (unsigned)expect_ysplit(h, M));
    // a tile with at most 1/SPARSE_DEN of its amplitudes non-zero is evaluated over the compacted list of those amplitudes
    constexpr int SPARSE_DEN = 4;
    const int sparse_den = dense_only ? (skip_diag ? -2 : -1) : ((H.d_agroups.p && sw.a1 > sw.a0) ? SPARSE_DEN : 0);
    if (int rc = lds_opt_in<&k_tile_expect<M, NT, true, REAL>, &k_tile_expect<M, NT, false, REAL>>(h, smem_full)) return rc;
    if (h->n_local >= 25) {
        hipLaunchKernelGGL((k_tile_expect<M, NT, true, REAL>), grid, dim3(NT), smem, stream, (const void *)h->state, h->base, sw,
                           (const ExChunkT *)H.d_tchunks.p, (const ExEntryT *)H.d_tgroups.p,
                           (const ExTermT *)H.d_tterms.p, (const ExFlatT *)H.d_tflats.p, (const ExItemT *)H.d_titems.p, partials,
                           accumulate, (const ExChunkT *)H.d_achunks.p, (const ExAGroupT *)H.d_agroups.p,
                           (const ExTermT *)H.d_aterms.p, sparse_den, census);
    } else {
        hipLaunchKernelGGL((k_tile_expect<M, NT, false, REAL>), grid, dim3(NT), smem, stream, (const void *)h->state, h->base, sw,
                           (const ExChunkT *)H.d_tchunks.p, (const ExEntryT *)H.d_tgroups.p,
                           (const ExTermT *)H.d_tterms.p, (const ExFlatT *)H.d_tflats.p, (const ExItemT *)H.d_titems.p, partials,
                           accumulate, (const ExChunkT *)H.d_achunks.p, (const ExAGroupT *)H.d_agroups.p,
                           (const ExTermT *)H.d_aterms.p, sparse_den, census);
    }
    HIPC(h, hipGetLastError());
    return OVQE_OK;
}

// <state|H|state> of the stored Hamiltonian through the tile cover; *used = false when there is no cover
int run_expectation_tiled(ovqe_handle h, HamDev &H, double2 *out, bool *used, bool real = false) {
    *used = false;
    if (H.tile_bits != tile_bits(h, real) || H.tile_low != HAM_TILE_LOW || H.tile_real != real) {
        int rc = build_ham_tiles(h, H, real);
        if (rc) return rc;
    }
    if (H.tsweeps.empty() && !(real && H.n_rest)) return OVQE_OK;
    const int M = H.tile_bits;
    // partial sums: one per workgroup of the tile sweeps (none when every group keeps its own sweep)
    const int64_t ntiles = H.tsweeps.empty() ? 0 : (int64_t)(h->namps >> M) * expect_ysplit(h, M);
    const int nb = reduce_blocks(h->namps);
    const int64_t ndiag = H.diag_nu > 0 ? (int64_t)(h->namps >> H.diag_bits) : 0;   // workgroups of k_tile_diag (dense registers)
    int rc = ensure(h, h->d_partials, (size_t)(2 * ntiles + nb + ndiag) * sizeof(double2));
    if (rc) return rc;
    rc = ensure(h, h->d_result, 64 * sizeof(double2));
    if (rc) return rc;
    double2 *partials = (double2 *)h->d_partials.p;
    // two streams when the cover has enough sweeps: the sweeps are taken heaviest-first by the main stream and
    // lightest-first by the second one until they meet (estimated duration: one read of the state + compute per term)
    const int ns = (int)H.tsweeps.size();
    // (shards too: the second stream forks from and joins the handle's stream by events, so what the caller ordered behind that
    // stream — the RCCL transfers of the partitioned register — stays ordered behind both)
    const bool dual = ns >= 8 && h->n_local >= 20;
    if (dual && !h->stream2) {
        HIPC(h, hipStreamCreateWithFlags(&h->stream2, hipStreamNonBlocking));
        HIPC(h, hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
        HIPC(h, hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming));
    }
    std::vector<char> on_second(ns, 0);
    int acc[2] = {0, 0};
    // Dense complex registers of 25+ qubits (a shard of the partitioned register, a random state): the LDS that the sparse-tile path
    // needs beside a 64-KB tile leaves ONE workgroup per CU, which then loads, waits and computes in turn (31 qubits: 62 sweeps at
    // 1.1 TB/s).  The first sweep of an evaluation counts the tiles that took the sparse path; when none did, the state is dense
    // under every tile bit set and the remaining sweeps run without that area: two workgroups per CU, of either stream.  (One stream
    // synchronisation per evaluation: only where there are at least four sweeps of at least half a gigabyte.)
    // (round 6: real states too — the float64 shards of the partitioned register: tiles of 2^13 doubles)
    const bool try_dense = ((!real && M == 12) || (real && M == 13)) && h->n_local >= 25 && ns >= 4 && h->opt_expect_dense;
    bool dense_only = false;
    int census_k = -1;      // the sweep that ran first, as the census
    if (try_dense) {
        rc = ensure(h, h->d_tile_cnt, sizeof(int));
        if (rc) return rc;
        // (the census takes a sweep WITHOUT the diagonal group when that group has a Walsh-Hadamard form: on a dense register the
        // group's hundreds of strings then never run term by term)
        census_k = (ndiag && H.diag_sweep == 0 && ns > 1) ? 1 : 0;
        HIPC(h, hipMemsetAsync(h->d_tile_cnt.p, 0, sizeof(int), h->stream));
        rc = real ? launch_tile_expect<13, true>(h, H, H.tsweeps[census_k], partials, 0, h->stream, false, (int *)h->d_tile_cnt.p)
                  : launch_tile_expect<12, false>(h, H, H.tsweeps[census_k], partials, 0, h->stream, false, (int *)h->d_tile_cnt.p);
        if (rc) return rc;
        int census = 1;
        HIPC(h, hipMemcpyAsync(&census, h->d_tile_cnt.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIPC(h, hipStreamSynchronize(h->stream));
        dense_only = census == 0;
        acc[0] = 1;
    }
    const bool diag_wht = dense_only && ndiag > 0 && H.diag_sweep != census_k;
    if (dual) {
        const double mem = 16.0 * (double)h->namps * (real ? 0.5 : 1.0) / 2.8e6;        // us at ~2.8 TB/s
        const double per_term = 0.23 * (double)h->namps / (double)(1ull << 24);       // us, measured at 24 qubits
        double ta = 0.0, tb = 0.0;
        int i = 0, j = ns - 1;
        while (i <= j) {
            if (ta <= tb) ta += mem + per_term * H.tsweep_terms[i++];
            else {
                tb += mem + per_term * H.tsweep_terms[j];
                on_second[j--] = 1;
            }
        }
        HIPC(h, hipEventRecord(h->ev_fork, h->stream));
        HIPC(h, hipStreamWaitEvent(h->stream2, h->ev_fork, 0));
    }
    for (int k = 0; k < ns; ++k) {
        if (k == census_k) continue;
        const ExSweep &sw = H.tsweeps[k];
        const int which = on_second[k];
        hipStream_t strm = which ? h->stream2 : h->stream;
        double2 *part = partials + (which ? ntiles : 0);
        if (real) {
            switch (M) {
            case 11: rc = launch_tile_expect<11, true>(h, H, sw, part, acc[which], strm); break;
            case 12: rc = launch_tile_expect<12, true>(h, H, sw, part, acc[which], strm); break;
            default: rc = launch_tile_expect<13, true>(h, H, sw, part, acc[which], strm, dense_only, nullptr, diag_wht); break;
            }
        } else {
            switch (M) {
            case 10: rc = launch_tile_expect<10, false>(h, H, sw, part, acc[which], strm); break;
            case 11: rc = launch_tile_expect<11, false>(h, H, sw, part, acc[which], strm); break;
            default: rc = launch_tile_expect<12, false>(h, H, sw, part, acc[which], strm, dense_only, nullptr, diag_wht); break;
            }
        }
        if (rc) return rc;
        acc[which] = 1;
    }
    const int nparts = (dual && acc[1]) ? 2 : 1;
    if (dual) {
        HIPC(h, hipEventRecord(h->ev_join, h->stream2));
        HIPC(h, hipStreamWaitEvent(h->stream, h->ev_join, 0));
    }
    int64_t count = ntiles * nparts;
    if (diag_wht) {   // the diagonal group: one pass over contiguous tiles, Walsh-Hadamard form (sv_tile.hpp k_tile_diag)
        constexpr int DM = 12, DNT = 512;
        constexpr size_t dsm = tile_diag_lds<DM, DNT>().bytes;
        const bool ntl = h->n_local >= 25;
        if (real) {
            if (ntl) hipLaunchKernelGGL((k_tile_diag<DM, DNT, true, true>), dim3((unsigned)ndiag), dim3(DNT), dsm, h->stream, (const void *)h->state, h->base,
                                        (const uint32_t *)H.d_dzin.p, (const int32_t *)H.d_doff.p, (const DiagTermT *)H.d_dterms.p, H.diag_nu, partials + count, 0);
            else hipLaunchKernelGGL((k_tile_diag<DM, DNT, false, true>), dim3((unsigned)ndiag), dim3(DNT), dsm, h->stream, (const void *)h->state, h->base,
                                    (const uint32_t *)H.d_dzin.p, (const int32_t *)H.d_doff.p, (const DiagTermT *)H.d_dterms.p, H.diag_nu, partials + count, 0);
        } else {
            if (ntl) hipLaunchKernelGGL((k_tile_diag<DM, DNT, true, false>), dim3((unsigned)ndiag), dim3(DNT), dsm, h->stream, (const void *)h->state, h->base,
                                        (const uint32_t *)H.d_dzin.p, (const int32_t *)H.d_doff.p, (const DiagTermT *)H.d_dterms.p, H.diag_nu, partials + count, 0);
            else hipLaunchKernelGGL((k_tile_diag<DM, DNT, false, false>), dim3((unsigned)ndiag), dim3(DNT), dsm, h->stream, (const void *)h->state, h->base,
                                    (const uint32_t *)H.d_dzin.p, (const int32_t *)H.d_doff.p, (const DiagTermT *)H.d_dterms.p, H.diag_nu, partials + count, 0);
        }
        count += ndiag;
    }
    if (H.n_rest) {
        if (real)
            hipLaunchKernelGGL(k_expect_pairs_real, dim3(nb), dim3(256), 0, h->stream, (const double *)h->state, h->namps,
                               (const HGroup *)H.d_rest.p, 0, H.n_rest, (const HTerm *)H.d_terms.p, partials + count);
        else
            hipLaunchKernelGGL(k_expect_pairs, dim3(nb), dim3(256), 0, h->stream, h->state, h->namps,
                               (const HGroup *)H.d_rest.p, 0, H.n_rest, (const HTerm *)H.d_terms.p, partials + count);
        count += nb;
    }
    if (int rc = reduce_to_host(h, partials, count, out)) return rc;
    *used = true;
    h->last_passes = ns + (H.n_rest ? 1 : 0);
    h->last_pass_bytes = (int64_t)((real ? 8.0 : 16.0) * (double)h->namps * (double)(ns + H.n_rest));
    return OVQE_OK;
}

// ---- compact cover -----------------------------------------------------------------------------------------------
int run_program_streaming(ovqe_handle h, const double *theta, bool real);

// Support of the program's states (non-zeros of the real state prepared at a generic parameter vector: structural zeros
// are exact zeros for every theta, and a structurally non-zero amplitude vanishes exactly only on a null set) and, for
// every sweep of the real cover, that support sorted by tile.  Clobbers the state buffer.
int build_compact_cover(ovqe_handle h, HamDev &H) {
    CompactCover &C = h->cc;
    C.valid = false;
    C.disabled = true;   // until everything below succeeded
    C.prog_version = h->prog_version;
    C.ham_version = H.version;
    C.cover_id = H.cover_id;
    const int M = H.tile_bits;
    if (H.tsweeps.empty() || H.n_rest || !H.tile_real || h->n_local > 28 || M > 13) return OVQE_OK;
    std::vector<double> theta((size_t)std::max(h->K, 1));
    for (int k = 0; k < h->K; ++k) {
        const double f = 0.6180339887498949 * (k + 1);
        theta[k] = 0.4 + 0.7 * (f - std::floor(f));
    }
    int rc = run_program_streaming(h, theta.data(), true);
    if (rc) return rc;
    std::vector<double> host(h->namps);
    HIPC(h, hipMemcpyAsync(host.data(), h->state, h->namps * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    std::vector<uint32_t> sup;
    for (uint64_t i = 0; i < h->namps; ++i)
        if (host[i] != 0.0) sup.push_back((uint32_t)i);
    std::vector<double>().swap(host);
    const uint32_t K = (uint32_t)sup.size();
    if (K == 0 || (uint64_t)K * 8ull > h->namps) return OVQE_OK;   // not sparse enough to pay off
    const int ns = (int)H.tsweeps.size();
    const uint64_t ntiles = h->namps >> M;
    std::vector<uint16_t> loc((size_t)ns * K);
    std::vector<uint32_t> cid((size_t)ns * K), off((size_t)ns * (ntiles + 1));
    std::vector<uint32_t> maxn(ns, 0);
    const uint64_t allbits = h->namps - 1ull;
    auto work = [&](int s0, int s1) {
        std::vector<uint32_t> cnt(ntiles + 1), tile_of(K);
        for (int s = s0; s < s1; ++s) {
            const uint64_t samp = (H.tsweeps[s].smask << 1) | 1ull;   // the tile's bits in amplitude-index space
            const uint64_t outside = allbits & ~samp;
            // byte tables of the two bit extractions
            uint32_t tl[4][256], tt[4][256];
            for (int b = 0; b < 4; ++b) {
                const uint64_t ms = (samp >> (8 * b)) & 0xffull, mo = (outside >> (8 * b)) & 0xffull;
                const int sh_s = __builtin_popcountll(samp & ((1ull << (8 * b)) - 1ull));
                const int sh_o = __builtin_popcountll(outside & ((1ull << (8 * b)) - 1ull));
                for (int v = 0; v < 256; ++v) {
                    tl[b][v] = extract_bits((uint64_t)v, ms) << sh_s;
                    tt[b][v] = extract_bits((uint64_t)v, mo) << sh_o;
                }
            }
            std::fill(cnt.begin(), cnt.end(), 0u);
            for (uint32_t k = 0; k < K; ++k) {
                const uint32_t i = sup[k];
                const uint32_t t = tt[0][i & 255u] | tt[1][(i >> 8) & 255u] | tt[2][(i >> 16) & 255u] | tt[3][i >> 24];
                tile_of[k] = t;
                cnt[t + 1]++;
            }
            uint32_t mx = 0;
            for (uint64_t t = 0; t < ntiles; ++t) {
                mx = std::max(mx, cnt[t + 1]);
                cnt[t + 1] += cnt[t];
            }
            maxn[s] = mx;
            uint32_t *o = off.data() + (size_t)s * (ntiles + 1);
            std::copy(cnt.begin(), cnt.end(), o);
            uint16_t *L = loc.data() + (size_t)s * K;
            uint32_t *Cd = cid.data() + (size_t)s * K;
            for (uint32_t k = 0; k < K; ++k) {   // ascending k inside a tile: a stable order
                const uint32_t i = sup[k];
                const uint32_t l = tl[0][i & 255u] | tl[1][(i >> 8) & 255u] | tl[2][(i >> 16) & 255u] | tl[3][i >> 24];
                const uint32_t pos = cnt[tile_of[k]]++;
                L[pos] = (uint16_t)l;
                Cd[pos] = k;   // compact id of the element at this tile-sorted position
            }
        }
    };
    {
        const int nthr = std::max(1, std::min<int>({ns, 16, (int)std::thread::hardware_concurrency()}));
        std::vector<std::thread> pool;
        for (int t = 0; t < nthr; ++t) pool.emplace_back(work, (int)((int64_t)ns * t / nthr), (int)((int64_t)ns * (t + 1) / nthr));
        for (std::thread &t : pool) t.join();
    }
    rc = upload(h, C.d_sup, sup.data(), (size_t)K * sizeof(uint32_t));
    if (!rc) rc = upload(h, C.d_loc, loc.data(), loc.size() * sizeof(uint16_t));
    if (!rc) rc = upload(h, C.d_cid, cid.data(), cid.size() * sizeof(uint32_t));
    if (!rc) rc = upload(h, C.d_off, off.data(), off.size() * sizeof(uint32_t));
    if (!rc) rc = ensure(h, C.d_psic, ((size_t)ns + 1) * K * sizeof(double));   // [compact state][per-sweep tile order]
    if (!rc) rc = upload(h, C.d_sweeps, H.tsweeps.data(), (size_t)ns * sizeof(ExSweep));
    if (rc) return rc;
    C.K = K;
    C.ntiles = ntiles;
    C.max_nnz = *std::max_element(maxn.begin(), maxn.end());
    C.valid = true;
    C.disabled = false;
    return OVQE_OK;
}

template <int M>
int launch_tile_expect_compact(ovqe_handle h, const HamDev &H, double2 *partials) {
    constexpr int NT = 1 << TILE_EXPECT_LOG_NT;
    const CompactCover &C = h->cc;
    constexpr int cpp = 1;   // host chunks (512 terms each) staged in LDS per pass
    const int term_cap = cpp * TILE_TERM_CAP, group_cap = cpp * TILE_APPLY_GROUPS;
    const size_t smem = tile_compact_lds<M, NT, true>(term_cap, group_cap, (uint32_t)C.max_nnz).bytes;
    if (int rc = lds_opt_in<&k_tile_expect_compact<M, NT, true>>(h, 120 * 1024)) return rc;
    hipLaunchKernelGGL((k_tile_expect_compact<M, NT, true>), dim3((unsigned)C.ntiles, (unsigned)H.tsweeps.size()), dim3(NT),
                       smem, h->stream, (const double *)C.d_psic.p + C.K, (const uint16_t *)C.d_loc.p, (const uint32_t *)C.d_off.p,
                       h->base, (const ExSweep *)C.d_sweeps.p, C.K, (const ExChunkT *)H.d_achunks.p,
                       (const ExAGroupT *)H.d_agroups.p, (const ExTermT *)H.d_aterms.p, partials, term_cap, group_cap, cpp);
    HIPC(h, hipGetLastError());
    return OVQE_OK;
}

// <state|H|state> of a real state through the compact cover; *ok = false when the guard failed (support not closed)
int run_expectation_compact(ovqe_handle h, HamDev &H, double2 *out, bool *ok, bool psic_ready = false) {
    CompactCover &C = h->cc;
    *ok = false;
    const int ns = (int)H.tsweeps.size();
    const uint64_t total = (uint64_t)ns * C.K;
    const int nbg = (int)std::min<uint32_t>(2048u, (C.K + 255u) / 256u);
    const size_t nslots = (size_t)ns * C.ntiles;
    int rc = ensure(h, h->d_partials, (nslots + (size_t)ns + nbg) * sizeof(double2));
    if (!rc) rc = ensure(h, h->d_result, 64 * sizeof(double2));
    if (rc) return rc;
    double2 *partials = (double2 *)h->d_partials.p, *rows = partials + nslots, *pnorm = rows + ns;
    if (!psic_ready)   // (else the sector path's circuit left the compact state in C.d_psic: nothing to gather, norm 1 by construction)
        hipLaunchKernelGGL(k_compact_gather<true>, dim3(nbg), dim3(256), 0, h->stream, (const double *)h->state,
                           (const uint32_t *)C.d_sup.p, C.K, (double *)C.d_psic.p, pnorm);
    hipLaunchKernelGGL(k_compact_permute<true>, dim3((unsigned)std::min<uint64_t>(16384u, (total + 255u) / 256u)), dim3(256), 0,
                       h->stream, (const double *)C.d_psic.p, (const uint32_t *)C.d_cid.p, total, (double *)C.d_psic.p + C.K);
    switch (H.tile_bits) {
    case 11: rc = launch_tile_expect_compact<11>(h, H, partials); break;
    case 12: rc = launch_tile_expect_compact<12>(h, H, partials); break;
    default: rc = launch_tile_expect_compact<13>(h, H, partials); break;
    }
    if (rc) return rc;
    // fixed-order reduction: per sweep over its tiles, then over the sweeps
    hipLaunchKernelGGL(k_reduce_rows2, dim3((unsigned)ns), dim3(256), 0, h->stream, (const double2 *)partials, (int)C.ntiles, rows);
    rc = enqueue_reduce(h, rows, ns);
    if (!rc && !psic_ready) rc = enqueue_reduce(h, pnorm, nbg, 1);
    double2 sums[2];   // <H>, norm on the support
    if (!rc) rc = fetch_result(h, sums, 2);
    if (rc) return rc;
    // guard: the circuit is unitary, so the amplitudes on the support must carry the whole norm
    if (!psic_ready && std::fabs(sums[1].x - 1.0) > 1e-9) return OVQE_OK;
    *out = sums[0];
    *ok = true;
    return OVQE_OK;
}

// out = ident * in + H in for the stored Hamiltonian: tile sweeps when the cover holds every group, else the gather
// kernel.  in / out: complex states of this handle's size, out != in.
template <int M>
int launch_tile_apply(ovqe_handle h, const HamDev &H, const ExSweep &sw, const amp_t *in, amp_t *out, int first,
                      double ident, const uint32_t *tile_list = nullptr, const uint32_t *tile_count = nullptr,
                      unsigned listed_grid = 0) {
    constexpr int NT = 1 << TILE_EXPECT_LOG_NT;  // the sweeps' thread / trip masks are laid out for this group size
    constexpr size_t smem = tile_apply_lds<M>(sizeof(double2), 0).bytes;
    if (int rc = lds_opt_in<&k_tile_apply<M, NT, true>, &k_tile_apply<M, NT, false>>(h, smem)) return rc;
    const unsigned grid = tile_list ? listed_grid : (unsigned)(h->namps >> M);
    if (h->n_local >= 25) {
        hipLaunchKernelGGL((k_tile_apply<M, NT, true>), dim3(grid), dim3(NT), smem, h->stream, in, out, h->base, sw,
                           (const ExChunkT *)H.d_achunks.p, (const ExAGroupT *)H.d_agroups.p,
                           (const ExTermT *)H.d_aterms.p, first, ident, tile_list, tile_count);
    } else {
        hipLaunchKernelGGL((k_tile_apply<M, NT, false>), dim3(grid), dim3(NT), smem, h->stream, in, out, h->base, sw,
                           (const ExChunkT *)H.d_achunks.p, (const ExAGroupT *)H.d_agroups.p,
                           (const ExTermT *)H.d_aterms.p, first, ident, tile_list, tile_count);
    }
    HIPC(h, hipGetLastError());
    return OVQE_OK;
}

// in_idx / in_count: the ascending list of the non-zero amplitudes of `in` when the caller has it (the ADAPT screen of a
// state of a few determinants): every sweep then only visits the tiles that hold one of them
int apply_hamiltonian(ovqe_handle h, amp_t *out, const amp_t *in, double ident, const uint64_t *in_idx = nullptr,
                      uint64_t in_count = 0, HamDev *which = nullptr) {
    HamDev &H = which ? *which : h->ham;   // (which: the local part of a planned cross-shard sum, cross_host.inc)
    if (H.tile_bits != tile_bits(h, false) || H.tile_low != HAM_TILE_LOW || H.tile_real) {
        int rc = build_ham_tiles(h, H, false);
        if (rc) return rc;
    }
    // below ~2^8 tiles the tile sweeps leave most of the chip idle: the gather kernel (state in L2) is faster there
    if (H.tsweeps.empty() || H.n_rest || (int64_t)(h->namps >> H.tile_bits) < h->opt_apply_min_tiles) {
        hipLaunchKernelGGL(k_apply_sum, dim3(reduce_blocks(h->namps)), dim3(256), 0, h->stream, out, in, (amp_t *)nullptr,
                           h->namps, h->base, (const HGroup *)H.d_groups.p, (int)H.groups.size(),
                           (const HTerm *)H.d_terms.p, 1.0, 0.0, ident, 0.0);
        HIPC(h, hipGetLastError());
        return OVQE_OK;
    }
    const uint32_t *lists = nullptr, *counts = nullptr;
    const uint64_t ntiles = h->namps >> H.tile_bits;
    uint32_t cap = 0;
    if (in_idx && in_count > 0 && ntiles <= (1u << 19) && in_count * 4 <= ntiles) {
        const size_t nsw = H.tsweeps.size();
        cap = (uint32_t)std::min<uint64_t>(in_count, ntiles);
        std::vector<uint64_t> smasks(nsw);
        for (size_t k = 0; k < nsw; ++k) smasks[k] = H.tsweeps[k].smask;
        int rc = upload(h, h->d_tile_smasks, smasks.data(), nsw * sizeof(uint64_t));
        if (!rc) rc = ensure(h, h->d_tile_lists, nsw * (size_t)cap * sizeof(uint32_t));
        if (!rc) rc = ensure(h, h->d_tile_counts, nsw * sizeof(uint32_t));
        if (rc) return rc;
        HIPC(h, hipMemsetAsync(out, 0, h->namps * sizeof(amp_t), h->stream));
        hipLaunchKernelGGL(k_tile_lists, dim3((unsigned)nsw), dim3(256), (size_t)((ntiles + 31) / 32) * sizeof(uint32_t), h->stream,
                           in_idx, in_count, (const uint64_t *)h->d_tile_smasks.p, h->n_local, (uint32_t)ntiles, cap,
                           (uint32_t *)h->d_tile_lists.p, (uint32_t *)h->d_tile_counts.p);
        HIPC(h, hipGetLastError());
        lists = (const uint32_t *)h->d_tile_lists.p;
        counts = (const uint32_t *)h->d_tile_counts.p;
    }
    int first = 1;
    size_t k = 0;
    for (const ExSweep &sw : H.tsweeps) {
        const uint32_t *tl = lists ? lists + k * cap : nullptr, *tc = lists ? counts + k : nullptr;
        int rc;
        switch (H.tile_bits) {
        case 10: rc = launch_tile_apply<10>(h, H, sw, in, out, first, ident, tl, tc, cap); break;
        case 11: rc = launch_tile_apply<11>(h, H, sw, in, out, first, ident, tl, tc, cap); break;
        default: rc = launch_tile_apply<12>(h, H, sw, in, out, first, ident, tl, tc, cap); break;
        }
        if (rc) return rc;
        first = 0;
        ++k;
    }
    return OVQE_OK;
}

int init_basis(ovqe_handle h, uint64_t index, double2 one = make_double2(1.0, 0.0)) {
    const uint64_t lmask = local_mask(h);
    const int has = ((index & ~lmask) == h->base) ? 1 : 0;
    hipLaunchKernelGGL(k_init_basis, dim3(reduce_blocks(h->namps)), dim3(256), 0, h->stream, h->state, h->namps,
                       index & lmask, has, one);
    HIPC(h, hipGetLastError());
    return OVQE_OK;
}

// ---- LDS-tiled multi-op sweeps (sv_tile.hpp) --------------------------------------------------------
template <int M, bool REAL>
int launch_tile(ovqe_handle h, const TilePlan &tp, const TileSeg &sg) {
    constexpr int NT = 1 << TILE_SWEEP_LOG_NT;
    constexpr size_t smem = tile_sweep_lds<M, REAL>().bytes;
    const unsigned grid = (unsigned)(h->namps >> M);
    const bool ntl = h->n_local >= 25;
    if (int rc = lds_opt_in<&k_tile_sweep<M, NT, true, REAL>, &k_tile_sweep<M, NT, false, REAL>>(h, smem)) return rc;
    if (ntl) {
        hipLaunchKernelGGL((k_tile_sweep<M, NT, true, REAL>), dim3(grid), dim3(NT), smem, h->stream, (void *)h->state,
                           h->base, sg, (const TileOp *)tp.d_tops.p, (const TileRot *)tp.d_trots.p,
                           (const RotParam *)h->d_rp.p);
    } else {
        hipLaunchKernelGGL((k_tile_sweep<M, NT, false, REAL>), dim3(grid), dim3(NT), smem, h->stream, (void *)h->state,
                           h->base, sg, (const TileOp *)tp.d_tops.p, (const TileRot *)tp.d_trots.p,
                           (const RotParam *)h->d_rp.p);
    }
    HIPC(h, hipGetLastError());
    return OVQE_OK;
}

// tile sizes: complex 2^10..2^12 amplitudes; real 2^11..2^13 (the segment's masks then hold one bit less, sv_tile.hpp)
int launch_tile_segment(ovqe_handle h, const TilePlan &tp, const TileSeg &sg, bool real = false) {
    const int bits = __builtin_popcountll(sg.smask) + (real ? 1 : 0);
    if (real) {
        switch (bits) {
        case 11: return launch_tile<11, true>(h, tp, sg);
        case 12: return launch_tile<12, true>(h, tp, sg);
        case 13: return launch_tile<13, true>(h, tp, sg);
        }
    } else {
        switch (bits) {
        case 10: return launch_tile<10, false>(h, tp, sg);
        case 11: return launch_tile<11, false>(h, tp, sg);
        case 12: return launch_tile<12, false>(h, tp, sg);
        }
    }
    return fail(h, OVQE_ERR_INVALID, "corrupt tile segment");
}

// backward twin (k_tile_adjoint): psi and lam tiles of 2^M amplitudes, a grid sized to the CUs whose workgroups walk the tiles
// (adjoint_tile_grid) -> partials[(r - sg.rot0) * grid + workgroup]
inline int adjoint_tile_bits(ovqe_handle h) {
    const int m = h->opt_adjoint_tile_bits >= 0 ? h->opt_adjoint_tile_bits : (h->n_local >= 25 ? 12 : 11);
    return (m == 11 || m == 12) && h->n_local >= m + 2 ? m : 0;   // 0: the streaming kernels only
}
inline int adjoint_tile_grid(ovqe_handle h, int m) {
    handle_num_cus(h);
    return (int)std::min<uint64_t>(h->namps >> m, (uint64_t)h->num_cus * (m >= 12 ? 1 : 2));
}
template <int M>
int launch_tile_adjoint_m(ovqe_handle h, amp_t *lam, const TilePlan &tp, const TileSeg &sg, double *partials, int grid) {
    constexpr int NT = 1 << TILE_ADJ_LOG_NT;
    constexpr int CAP = tile_adj_rot_cap(M);
    constexpr size_t smem = tile_adjoint_lds<M, NT>().bytes;
    const bool ntl = h->n_local >= 25;
    if (int rc = lds_opt_in<&k_tile_adjoint<M, NT, true>, &k_tile_adjoint<M, NT, false>>(h, smem)) return rc;
    const uint32_t ntiles = (uint32_t)(h->namps >> M);
    if (ntl) {
        hipLaunchKernelGGL((k_tile_adjoint<M, NT, true>), dim3((unsigned)grid), dim3(NT), smem, h->stream, h->state, lam, h->base,
                           ntiles, sg, (const TileOp *)tp.d_tops.p, (const TileRot *)tp.d_trots.p, (const RotParam *)h->d_rp.p,
                           partials);
    } else {
        hipLaunchKernelGGL((k_tile_adjoint<M, NT, false>), dim3((unsigned)grid), dim3(NT), smem, h->stream, h->state, lam, h->base,
                           ntiles, sg, (const TileOp *)tp.d_tops.p, (const TileRot *)tp.d_trots.p, (const RotParam *)h->d_rp.p,
                           partials);
    }
    HIPC(h, hipGetLastError());
    return OVQE_OK;
}

int launch_tile_adjoint(ovqe_handle h, amp_t *lam, const TilePlan &tp, const TileSeg &sg, double *partials, int grid) {
    for (int o = sg.op0; o < sg.op1; ++o)
        if (tp.tops[o].kind != OP_PAIR && tp.tops[o].kind != OP_DIAG) return fail(h, OVQE_ERR_INVALID, "corrupt tile segment");
    switch (__builtin_popcountll(sg.smask)) {
    case 11: return launch_tile_adjoint_m<11>(h, lam, tp, sg, partials, grid);
    case 12: return launch_tile_adjoint_m<12>(h, lam, tp, sg, partials, grid);
    }
    return fail(h, OVQE_ERR_INVALID, "corrupt tile segment");
}

// Greedy segmentation of the (table-fused) program into tile sweeps: consecutive ops are taken while the union of
// their mixing bits (x mask / gate target) and the mandatory low bits fits the tile; ops that do not fit, and
// segments of a single op, keep their own full-bandwidth sweep.  Commuting runs enter a tile in their OP_TAB form
// (one rotation per active pair pattern, see try_table_op): inside a fused sweep the arithmetic, not HBM, is the
// cost, and the table form does 1/64 of it for a JW double excitation.
// ``tile_m`` > 0: cut for a kernel with tiles of 2^tile_m amplitudes and ``rot_cap`` table entries instead of the forward
// sweep's (the backward kernel keeps two tiles in LDS: launch_tile_adjoint).
int build_tile_plan(ovqe_handle h, const std::vector<SmallOp> &sops, const std::vector<SmallRot> &srots,
                    const std::vector<uint64_t> &sop_zc, TilePlan &tp, bool real = false, int tile_m = 0,
                    int rot_cap = TILE_ROT_CAP) {
    tp.tsegs.clear();
    tp.tops.clear();
    tp.trots.assign(srots.size(), TileRot{0, 0, 0});
    tp.plan.clear();
    const int M = tile_m > 0 ? tile_m : tile_bits(h, real);
    const int nops = (int)sops.size();
    const bool tiled = tile_m > 0 ? (h->n_local >= M + 2 && h->opt_tile_low >= 0 && h->opt_tile_low <= 8) : tile_ok(h, real);
    if (!tiled) {
        for (int i = 0; i < nops; ++i) tp.plan.push_back(-1 - i);
        return OVQE_OK;
    }
    const uint64_t lowbits = (1ull << h->opt_tile_low) - 1ull;
    auto need = [&](const SmallOp &op) -> uint64_t {
        switch (op.kind) {
        case OP_PAIR:
        case OP_TAB: return op.x;
        case OP_DIAG: return 0ull;
        case OP_CNOT: return 1ull << op.count;
        default: return 1ull << op.pivot;
        }
    };
    auto is_rot = [](const SmallOp &op) { return op.kind == OP_PAIR || op.kind == OP_DIAG || op.kind == OP_TAB; };
    int i = 0;
    while (i < nops) {
        uint64_t S = lowbits;
        int j = i, nrot = 0;
        while (j < nops) {
            const SmallOp &op = sops[j];
            const uint64_t nb = S | need(op);
            if (__builtin_popcountll(nb) > M) break;
            if (is_rot(op) && nrot + op.count > rot_cap) break;
            if (is_rot(op)) nrot += op.count;
            S = nb;
            ++j;
        }
        if (j - i < 2) {
            tp.plan.push_back(-1 - i);
            ++i;
            continue;
        }
        for (int b = 0; __builtin_popcountll(S) < M; ++b) S |= 1ull << b;  // fill with the lowest free bits
        TileSeg sg = {};
        sg.smask = real ? S >> 1 : S;  // real state: masks in the index space of amplitude pairs
        uint64_t lo = 0, mk = sg.smask;
        for (int k = 0; k < TILE_SWEEP_LOG_NT; ++k) {  // thread bits
            lo |= mk & (0ull - mk);
            mk &= mk - 1ull;
        }
        sg.mask_lo = lo;
        sg.mask_hi = sg.smask & ~lo;
        sg.op0 = (int32_t)tp.tops.size();
        sg.rot0 = sg.rot1 = -1;
        for (int o = i; o < j; ++o) {
            const SmallOp &op = sops[o];
            TileOp t = {};
            t.kind = (int16_t)op.kind;
            if (is_rot(op)) {
                t.x = extract_bits(op.x, S);
                t.pivot = (int16_t)(t.x ? 31 - __builtin_clz(t.x) : 0);
                t.first = op.first;
                t.count = op.count;
                if (sg.rot0 < 0) sg.rot0 = op.first;
                sg.rot1 = op.first + op.count;
                const uint64_t zc = op.kind == OP_TAB ? sop_zc[o] : 0ull;
                t.zc = extract_bits(zc, S);
                for (int r = op.first; r < op.first + op.count; ++r) {
                    // OP_TAB entries: z = the pattern's bits (inside x, hence inside the tile); the run's common z
                    // part outside the tile is a per-tile sign of every entry
                    tp.trots[r].zin = extract_bits(srots[r].z, S);
                    tp.trots[r].zout = op.kind == OP_TAB ? (zc & ~S) : (srots[r].z & ~S);
                }
            } else if (op.kind == OP_CNOT) {
                const int cb = op.first, tbit = op.count;
                t.x = extract_bits(1ull << tbit, S);
                t.pivot = (int16_t)(31 - __builtin_clz(t.x));
                t.first = ((S >> cb) & 1ull) ? (31 - __builtin_clz(extract_bits(1ull << cb, S))) : (-1 - cb);
            } else {
                t.x = extract_bits(1ull << op.pivot, S);
                t.pivot = (int16_t)(31 - __builtin_clz(t.x));
            }
            tp.tops.push_back(t);
        }
        if (sg.rot0 < 0) sg.rot0 = sg.rot1 = 0;
        sg.op1 = (int32_t)tp.tops.size();
        tp.plan.push_back((int32_t)tp.tsegs.size());
        tp.tsegs.push_back(sg);
        i = j;
    }
    int rc = upload(h, tp.d_tops, tp.tops.data(), tp.tops.size() * sizeof(TileOp));
    if (rc) return rc;
    return upload(h, tp.d_trots, tp.trots.data(), tp.trots.size() * sizeof(TileRot));
}

int build_tile_program(ovqe_handle h) { return build_tile_plan(h, h->sops, h->srots, h->sop_zc, h->tp); }

inline RotParam resolve_rot(const SmallRot &sr, const double *theta) {
    const double phi = sr.phi0 + (sr.pidx >= 0 ? sr.coeff * theta[sr.pidx] : 0.0);
    RotParam rp;
    rp.z = sr.z;
    rp.c = std::cos(phi);
    const double s = std::sin(phi);
    rp.s = (sr.ny & 2) ? -s : s;
    rp.odd = sr.ny & 1;
    rp.pad = 0;
    return rp;
}

// Angle table of one evaluation in h->d_rp: [0, S) the entries of the table-fused program (tile sweeps, sequential runs),
// [S, S+R) the original rotations (commuting runs that keep their own sweep run in their sequential form).
int resolve_angles(ovqe_handle h, const double *theta, bool fused_only = false) {   // fused_only: [0, S) is all the caller reads (sector path)
    int rc = OVQE_OK;
    const size_t S = h->srots.size(), R = (fused_only && !h->probe_independent) ? 0 : h->rots.size();
    rc = ensure_rp(h, std::max<size_t>(S + R, 1));
    if (rc) return rc;
    static_assert(sizeof(RotSpec) == sizeof(SmallRot), "RotSpec mirrors SmallRot");
    if (h->probe_independent) {
        auto probe = [](const SmallRot &sr, size_t r) {
            const double f = 0.6180339887498949 * (double)(r + 1);
            const double phi = 0.4 + 0.7 * (f - std::floor(f));
            RotParam rp;
            rp.z = sr.z;
            rp.c = std::cos(phi);
            rp.s = (sr.ny & 2) ? -std::sin(phi) : std::sin(phi);
            rp.odd = sr.ny & 1;
            rp.pad = 0;
            return rp;
        };
        for (size_t r = 0; r < S; ++r) h->h_rp[r] = probe(h->srots[r], r);
        for (size_t r = 0; r < R; ++r) h->h_rp[S + r] = probe(h->rots[r], S + r);
        if (S + R)
            HIPC(h, hipMemcpyAsync(h->d_rp.p, h->h_rp, (S + R) * sizeof(RotParam), hipMemcpyHostToDevice, h->stream));
        return OVQE_OK;
    }
    if (S + h->rots.size() >= 256 && (size_t)h->K <= ovqe_sv::IO_DOUBLES && mapped_io(h, 1)) {
        // angles resolved on the device from the parameter vector (read through the pinned, mapped buffer): no host
        // trigonometry and no table upload on the evaluation path
        std::memcpy(h->h_io, theta, (size_t)h->K * sizeof(double));
        if (S)
            hipLaunchKernelGGL(k_resolve_rots, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, h->stream,
                               (const RotSpec *)h->d_rots.p, (int)S, (const double *)h->d_io, (RotParam *)h->d_rp.p);
        if (R)
            hipLaunchKernelGGL(k_resolve_rots, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, h->stream,
                               (const RotSpec *)h->d_rots_seq.p, (int)R, (const double *)h->d_io,
                               (RotParam *)h->d_rp.p + S);
    } else {
        for (size_t r = 0; r < S; ++r) h->h_rp[r] = resolve_rot(h->srots[r], theta);
        for (size_t r = 0; r < R; ++r) h->h_rp[S + r] = resolve_rot(h->rots[r], theta);
        if (S + R)
            HIPC(h, hipMemcpyAsync(h->d_rp.p, h->h_rp, (S + R) * sizeof(RotParam), hipMemcpyHostToDevice, h->stream));
    }
    return OVQE_OK;
}

// run the compiled program with the streaming kernels (state left in h->state).
// Angle table: [0, S) the entries of the table-fused program (tile sweeps, sequential runs), [S, S+R) the original
// rotations (commuting runs that keep their own sweep run in their sequential form).
int run_program_streaming(ovqe_handle h, const double *theta, bool real = false) {
    int rc = OVQE_OK;
    if (real) {
        if (!h->tp_real_built) {
            const auto t_plan = std::chrono::steady_clock::now();
            rc = build_tile_plan(h, h->sops, h->srots, h->sop_zc, h->tp_real, true);
            if (rc) return rc;
            h->tp_real_built = true;
            if (h->opt_sector_debug & 4)
                fprintf(stderr, "ovqe: tile plan of the real-amplitude program: %.2f ms\n",
                        1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t_plan).count());
        }
        hipLaunchKernelGGL(k_init_basis_real, dim3(reduce_blocks(h->namps)), dim3(256), 0, h->stream, (double *)h->state,
                           h->namps, h->hf);
    } else {
        rc = init_basis(h, h->hf, h->init_amp);
    }
    if (rc) return rc;
    const size_t S = h->srots.size();
    rc = resolve_angles(h, theta);
    if (rc) return rc;
    const RotParam *d_rp = (const RotParam *)h->d_rp.p;
    const TilePlan &tp = real ? h->tp_real : h->tp;
    const int nbr = reduce_blocks(h->namps);
    for (const int32_t step : tp.plan) {
        if (step >= 0) {
            rc = launch_tile_segment(h, tp, tp.tsegs[step], real);
            if (rc) return rc;
            continue;
        }
        const SmallOp &op = h->sops[-1 - step];
        if (real) {  // one-op sweeps on the real state
            double *st = (double *)h->state;
            if (op.kind == OP_PAIR) {
                hipLaunchKernelGGL(k_rot_pairs_real, dim3(nbr), dim3(256), 0, h->stream, st, h->namps >> 1, op.pivot, op.x,
                                   h->base, d_rp + op.first, op.count);
            } else if (op.kind == OP_TAB) {
                const SmallOp &src = h->ops[h->sop_src[-1 - step]];
                hipLaunchKernelGGL(k_rot_pairs_real, dim3(nbr), dim3(256), 0, h->stream, st, h->namps >> 1, src.pivot, src.x,
                                   h->base, d_rp + S + src.first, src.count);
            } else if (op.kind == OP_X || op.kind == OP_H) {
                hipLaunchKernelGGL(k_gate_real, dim3(nbr), dim3(256), 0, h->stream, st, h->namps >> 1,
                                   op.kind == OP_X ? 0 : 1, op.pivot, 0);
            } else if (op.kind == OP_CNOT) {
                hipLaunchKernelGGL(k_gate_real, dim3(nbr), dim3(256), 0, h->stream, st, h->namps >> 2, 2, op.first, op.count);
            } else {
                return fail(h, OVQE_ERR_INVALID, "internal: complex op in a real program");
            }
            continue;
        }
        switch (op.kind) {
        case OP_PAIR:
        case OP_DIAG:
            rc = launch_rot_run(h, op.kind == OP_PAIR ? op.x : 0ull, d_rp + op.first, op.count);
            break;
        case OP_TAB: {
            const SmallOp &src = h->ops[h->sop_src[-1 - step]];
            rc = launch_rot_run(h, src.x, d_rp + S + src.first, src.count);
            break;
        }
        case OP_X: rc = launch_gate(h, 0, op.pivot, 0); break;
        case OP_H: rc = launch_gate(h, 1, op.pivot, 0); break;
        case OP_CNOT: rc = launch_gate(h, 2, op.first, op.count); break;
        default: rc = fail(h, OVQE_ERR_INVALID, "corrupt program");
        }
        if (rc) return rc;
    }
    // the pinned table may be rewritten by the next call: make sure the copy has been consumed
    HIPC(h, hipStreamSynchronize(h->stream));
    return OVQE_OK;
}
