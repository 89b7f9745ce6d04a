// cross_host.inc — planned Pauli sums on one shard of the partitioned register: host planner and the ovqe_xsum_* entry points
// (kernels: sv_cross.hpp; the multi-rank protocol above them: openvqe_amd/distributed.py).  Included at the end of ovqe_sv.hip.
//
// Masks arrive in the PHYSICAL index-bit space of the whole register (n_local + n_global bits).  A term's x part on the rank bits,
// d = x >> n_local, names the partner shard (rank ^ d) its ket amplitudes live in; d = 0 terms act inside the shard.  The plan is
// made once per (Hamiltonian, permutation) — SURVEY.md section 8e: the same Hamiltonian is evaluated at every optimiser step
// (ref:openvqe/ucc_family/get_energy_ucc.py:46-48) and applied at every ADAPT macro-iteration
// (ref:openvqe/adapt/fermionic_adapt_vqe.py:114) — so an evaluation uploads nothing and synchronises once.

namespace {

// greedy cover of one partner's groups by (tile bit set inside the chunk, displacement outside it)
int build_cross_cover(ovqe_handle h, CrossCover &C, std::vector<CrossRawGroup> groups, int m, bool real) {
    if (real) {   // between real vectors a term with an imaginary folded coefficient (odd number of Y) contributes nothing
        for (CrossRawGroup &g : groups)
            g.terms.erase(std::remove_if(g.terms.begin(), g.terms.end(), [](const HTerm &t) { return t.ci != 0.0; }), g.terms.end());
        groups.erase(std::remove_if(groups.begin(), groups.end(), [](const CrossRawGroup &g) { return g.terms.empty(); }), groups.end());
    }
    C.ngroups = (int)groups.size();
    C.nterms = 0;
    for (const CrossRawGroup &g : groups) C.nterms += (int)g.terms.size();
    const uint64_t lowmask = (1ull << m) - 1ull;
    if (m < (real ? 11 : 10)) {   // too small to tile: classes of equal high x bits, one streaming launch each
        C.small = true;
        std::stable_sort(groups.begin(), groups.end(), [&](const CrossRawGroup &a, const CrossRawGroup &b) { return (a.x >> m) < (b.x >> m); });
        std::vector<HGroup> hg;
        std::vector<HTerm> ht;
        for (size_t g = 0; g < groups.size(); ++g) {
            const uint64_t hb = groups[g].x >> m;
            if (C.class_h.empty() || C.class_h.back() != hb) {
                C.class_h.push_back(hb);
                C.class_groups.push_back({(int)g, (int)g});
            }
            C.class_groups.back().second = (int)g + 1;
            HGroup gr = {};
            gr.x = groups[g].x & lowmask;
            gr.t0 = (int32_t)ht.size();
            ht.insert(ht.end(), groups[g].terms.begin(), groups[g].terms.end());
            gr.t1 = (int32_t)ht.size();
            hg.push_back(gr);
        }
        int rc = upload(h, C.d_groups, hg.data(), hg.size() * sizeof(HGroup));
        if (!rc) rc = upload(h, C.d_terms, ht.data(), ht.size() * sizeof(HTerm));
        return rc;
    }
    const int M = std::min(real ? 13 : 12, m);   // (a real tile holds 2^13 doubles in the same 64 KB; index bit 0 = the pair bit is always inside)
    C.M = M;
    const int L = std::min(HAM_TILE_LOW, M);
    const uint64_t lowbits = (1ull << L) - 1ull;
    const int G = (int)groups.size();
    std::vector<char> done(G, 0);
    int remaining = G;
    std::vector<ExChunkT> achunks;
    std::vector<ExAGroupT> agroups;
    std::vector<ExTermT> aterms;
    const double wgt[8] = {1.0, 0.25, 0.0625, 0.015625, 0.00390625, 0.0009765625, 0.000244140625, 0.00006103515625};
    while (remaining > 0) {
        // the class of high x bits with the most groups left fixes the part of d_out above the chunk
        std::map<uint64_t, int> per_class;
        for (int g = 0; g < G; ++g)
            if (!done[g]) ++per_class[groups[g].x >> m];
        uint64_t hb = 0;
        int best_n = -1;
        for (const auto &kv : per_class)
            if (kv.second > best_n) hb = kv.first, best_n = kv.second;
        // grow S over the chunk bits by the bit that brings the most groups of the class inside (build_ham_tiles' rule)
        uint64_t S = lowbits;
        while (__builtin_popcountll(S) < M) {
            const int room = M - __builtin_popcountll(S);
            double score[64] = {0.0};
            bool any = false;
            for (int g = 0; g < G; ++g) {
                if (done[g] || (groups[g].x >> m) != hb) continue;
                const uint64_t miss = groups[g].x & lowmask & ~S;
                const int nm = __builtin_popcountll(miss);
                if (nm == 0 || nm > room) continue;
                any = true;
                for (uint64_t mk = miss; mk; mk &= mk - 1ull) score[__builtin_ctzll(mk)] += wgt[std::min(nm - 1, 7)];
            }
            if (!any) break;
            int best = -1;
            for (int b = 0; b < m; ++b)
                if (!((S >> b) & 1ull) && (best < 0 || score[b] > score[best])) best = b;
            S |= 1ull << best;
        }
        for (int b = 0; __builtin_popcountll(S) < M; ++b) S |= 1ull << b;
        // the displacement below the chunk bits: the most frequent leftover (nothing left over whenever a group fits S)
        std::map<uint64_t, int> leftovers;
        for (int g = 0; g < G; ++g)
            if (!done[g] && (groups[g].x >> m) == hb) ++leftovers[groups[g].x & lowmask & ~S];
        uint64_t dl = 0;
        int dl_n = -1;
        for (const auto &kv : leftovers)
            if (kv.second > dl_n) dl = kv.first, dl_n = kv.second;   // (ascending keys: 0 wins a tie)
        CrossPass ps = {};
        ps.smask = real ? S >> 1 : S;   // real amplitudes: the kernel's masks live in the index space of amplitude PAIRS
        uint64_t lo = 0, mk = ps.smask;
        for (int k = 0; k < TILE_EXPECT_LOG_NT && mk; ++k) {
            lo |= mk & (0ull - mk);
            mk &= mk - 1ull;
        }
        ps.mask_lo = lo;
        ps.mask_hi = ps.smask & ~lo;
        ps.d_out = (hb << m) | dl;
        ps.a0 = (int32_t)achunks.size();
        ExChunkT ak = {(int32_t)agroups.size(), (int32_t)agroups.size(), (int32_t)aterms.size(), (int32_t)aterms.size()};
        int took = 0;
        for (int g = 0; g < G; ++g) {
            if (done[g] || (groups[g].x >> m) != hb || (groups[g].x & lowmask & ~S) != dl) continue;
            done[g] = 1;
            --remaining;
            ++took;
            const uint32_t xl = extract_bits(groups[g].x, S);
            const std::vector<HTerm> &ts = groups[g].terms;
            for (size_t k0 = 0; k0 < ts.size(); k0 += TILE_TERM_CAP) {   // (oversized groups in pieces: D_g is a sum over the terms)
                const size_t k1 = std::min(ts.size(), k0 + (size_t)TILE_TERM_CAP);
                if ((int)aterms.size() - ak.t0 + (int)(k1 - k0) > TILE_TERM_CAP || (int)agroups.size() - ak.g0 + 1 > TILE_APPLY_GROUPS) {
                    ak.g1 = (int32_t)agroups.size();
                    ak.t1 = (int32_t)aterms.size();
                    achunks.push_back(ak);
                    ak = {ak.g1, ak.g1, ak.t1, ak.t1};
                }
                ExAGroupT ag = {xl, (int32_t)aterms.size(), 0, 1};
                for (size_t k = k0; k < k1; ++k) {
                    ExTermT et = {};
                    et.zin = extract_bits(ts[k].z, S);
                    et.zout = ts[k].z & ~S;
                    et.cr = ts[k].cr;
                    et.ci = ts[k].ci;
                    if (et.ci != 0.0) ag.pad = 0;   // bit 0 of pad: every folded coefficient of the piece is real
                    aterms.push_back(et);
                }
                ag.t1 = (int32_t)aterms.size();
                agroups.push_back(ag);
            }
        }
        ak.g1 = (int32_t)agroups.size();
        ak.t1 = (int32_t)aterms.size();
        if (ak.g1 > ak.g0) achunks.push_back(ak);
        ps.a1 = (int32_t)achunks.size();
        if (took == 0) return fail(h, OVQE_ERR_INVALID, "internal: cross-shard cover made no progress");
        C.passes.push_back(ps);
    }
    int rc = upload(h, C.d_achunks, achunks.data(), achunks.size() * sizeof(ExChunkT));
    if (!rc) rc = upload(h, C.d_agroups, agroups.data(), agroups.size() * sizeof(ExAGroupT));
    if (!rc) rc = upload(h, C.d_aterms, aterms.data(), aterms.size() * sizeof(ExTermT));
    return rc;
}

template <int M, bool DOT>
int launch_tile_cross(ovqe_handle h, const CrossCover &C, const CrossPass &ps, const amp_t *ket, amp_t *other, uint64_t ket_gbase,
                      uint64_t chunk_off, unsigned grid, double2 *partials) {
    constexpr int NT = 1 << TILE_EXPECT_LOG_NT;
    constexpr size_t smem = tile_apply_lds<M>(sizeof(double2), NT / 64).bytes;
    if (int rc = lds_opt_in<&k_tile_cross<M, NT, true, DOT>, &k_tile_cross<M, NT, false, DOT>>(h, smem)) return rc;
    if (h->n_local >= 25)
        hipLaunchKernelGGL((k_tile_cross<M, NT, true, DOT>), dim3(grid), dim3(NT), smem, h->stream, ket, other, ket_gbase, chunk_off, ps,
                           (const ExChunkT *)C.d_achunks.p, (const ExAGroupT *)C.d_agroups.p, (const ExTermT *)C.d_aterms.p, partials);
    else
        hipLaunchKernelGGL((k_tile_cross<M, NT, false, DOT>), dim3(grid), dim3(NT), smem, h->stream, ket, other, ket_gbase, chunk_off, ps,
                           (const ExChunkT *)C.d_achunks.p, (const ExAGroupT *)C.d_agroups.p, (const ExTermT *)C.d_aterms.p, partials);
    HIPC(h, hipGetLastError());
    return OVQE_OK;
}

template <int M, bool DOT>
int launch_tile_cross_real(ovqe_handle h, const CrossCover &C, const CrossPass &ps, const double *ket, double *other, uint64_t ket_gbase,
                           uint64_t chunk_off, unsigned grid, double2 *partials) {
    constexpr int NT = 1 << TILE_EXPECT_LOG_NT;
    constexpr size_t smem = tile_apply_lds<M>(sizeof(double), NT / 64).bytes;
    if (int rc = lds_opt_in<&k_tile_cross_real<M, NT, true, DOT>, &k_tile_cross_real<M, NT, false, DOT>>(h, smem)) return rc;
    if (h->n_local >= 26)
        hipLaunchKernelGGL((k_tile_cross_real<M, NT, true, DOT>), dim3(grid), dim3(NT), smem, h->stream, ket, other, ket_gbase, chunk_off, ps,
                           (const ExChunkT *)C.d_achunks.p, (const ExAGroupT *)C.d_agroups.p, (const ExTermT *)C.d_aterms.p, partials);
    else
        hipLaunchKernelGGL((k_tile_cross_real<M, NT, false, DOT>), dim3(grid), dim3(NT), smem, h->stream, ket, other, ket_gbase, chunk_off, ps,
                           (const ExChunkT *)C.d_achunks.p, (const ExAGroupT *)C.d_agroups.p, (const ExTermT *)C.d_aterms.p, partials);
    HIPC(h, hipGetLastError());
    return OVQE_OK;
}

// the passes of cover C (real flavour) over one chunk of 2^m doubles; DOT: partials += other . (H_d ket), else other += H_d ket.
// A partner's cover takes the received chunks (m = the plan's chunk_bits); the d = 0 cover of sigma = H psi takes the shard itself
// as its one chunk (m = n_local, xsum_build_local).
template <bool DOT>
int run_cross_chunk_real(ovqe_handle h, CrossSum &X, const CrossCover &C, int m, uint64_t chunk, const double *ket, double *other) {
    const uint64_t csize = 1ull << m;
    const uint64_t ket_gbase = ((h->shard ^ C.d) << h->n_local) | (chunk << m);
    double2 *partials = (double2 *)X.d_part.p;
    if (C.small) {
        const int nb = (int)std::min<uint64_t>(DOT ? X.part_slots : 2048, std::max<uint64_t>(1, (csize + 255) / 256));
        for (size_t k = 0; k < C.class_h.size(); ++k)
            hipLaunchKernelGGL((k_cross_small_real<DOT>), dim3(nb), dim3(256), 0, h->stream, ket, other + ((chunk ^ C.class_h[k]) << m), csize,
                               ket_gbase, (const HGroup *)C.d_groups.p, C.class_groups[k].first, C.class_groups[k].second,
                               (const HTerm *)C.d_terms.p, partials);
        HIPC(h, hipGetLastError());
        return OVQE_OK;
    }
    const unsigned grid = (unsigned)(csize >> C.M);
    for (const CrossPass &ps : C.passes) {
        int rc;
        switch (C.M) {
        case 11: rc = launch_tile_cross_real<11, DOT>(h, C, ps, ket, other, ket_gbase, chunk << m, grid, partials); break;
        case 12: rc = launch_tile_cross_real<12, DOT>(h, C, ps, ket, other, ket_gbase, chunk << m, grid, partials); break;
        default: rc = launch_tile_cross_real<13, DOT>(h, C, ps, ket, other, ket_gbase, chunk << m, grid, partials); break;
        }
        if (rc) return rc;
    }
    return OVQE_OK;
}

// every pass of partner cover C over one received chunk; DOT: partials += conj(other) . (H_d ket), else other += H_d ket
template <bool DOT>
int run_cross_chunk(ovqe_handle h, CrossSum &X, const CrossCover &C, uint64_t chunk, const amp_t *ket, amp_t *other) {
    const int m = X.chunk_bits;
    const uint64_t csize = 1ull << m;
    const uint64_t ket_gbase = ((h->shard ^ C.d) << h->n_local) | (chunk << m);
    double2 *partials = (double2 *)X.d_part.p;
    if (C.small) {
        const int nb = (int)std::min<uint64_t>(X.part_slots, std::max<uint64_t>(1, (csize + 255) / 256));
        for (size_t k = 0; k < C.class_h.size(); ++k) {
            amp_t *oc = other + ((chunk ^ C.class_h[k]) << m);
            hipLaunchKernelGGL((k_cross_small<DOT>), dim3(nb), dim3(256), 0, h->stream, ket, oc, csize, ket_gbase, (const HGroup *)C.d_groups.p,
                               C.class_groups[k].first, C.class_groups[k].second, (const HTerm *)C.d_terms.p, partials);
        }
        HIPC(h, hipGetLastError());
        return OVQE_OK;
    }
    const unsigned grid = (unsigned)(csize >> C.M);
    for (const CrossPass &ps : C.passes) {
        int rc;
        switch (C.M) {
        case 10: rc = launch_tile_cross<10, DOT>(h, C, ps, ket, other, ket_gbase, chunk << m, grid, partials); break;
        case 11: rc = launch_tile_cross<11, DOT>(h, C, ps, ket, other, ket_gbase, chunk << m, grid, partials); break;
        default: rc = launch_tile_cross<12, DOT>(h, C, ps, ket, other, ket_gbase, chunk << m, grid, partials); break;
        }
        if (rc) return rc;
    }
    return OVQE_OK;
}

CrossSum *xsum_of(ovqe_handle h, int32_t id) {
    if (!h || id < 0 || id >= (int32_t)h->xsums.size() || !h->xsums[id]) {
        if (h) fail(h, OVQE_ERR_INVALID, "no such planned sum (ovqe_xsum_create)");
        return nullptr;
    }
    return h->xsums[id];
}

// the pass lists of every partner for complex (0) or real (1) amplitudes, built at the first use of that flavour
int xsum_build(ovqe_handle h, CrossSum &X, int real) {
    if (X.built[real]) return OVQE_OK;
    size_t slots = X.part_slots;
    X.partners[real].clear();
    X.partners[real].reserve(X.raw.size());
    for (const auto &kv : X.raw) {
        X.partners[real].emplace_back();
        CrossCover &C = X.partners[real].back();
        C.d = kv.first;
        int rc = build_cross_cover(h, C, kv.second, X.chunk_bits, real != 0);
        if (rc) return rc;
        slots = std::max<size_t>(slots, C.small ? (size_t)std::min<uint64_t>(2048, ((1ull << X.chunk_bits) + 255) / 256)
                                                : (size_t)1 << (X.chunk_bits - C.M));
    }
    if (slots > X.part_slots) {
        HIPC(h, hipStreamSynchronize(h->stream));
        int rc = ensure(h, X.d_part, slots * sizeof(double2));
        if (rc) return rc;
        X.part_slots = slots;
        HIPC(h, hipMemsetAsync(X.d_part.p, 0, slots * sizeof(double2), h->stream));
        HIPC(h, hipStreamSynchronize(h->stream));
    }
    X.built[real] = true;
    return OVQE_OK;
}

const CrossCover *xsum_partner(ovqe_handle h, CrossSum &X, uint64_t d, uint64_t chunk, int real) {
    if (chunk >> (h->n_local - X.chunk_bits)) {
        fail(h, OVQE_ERR_INVALID, "chunk index beyond the shard");
        return nullptr;
    }
    if (xsum_build(h, X, real)) return nullptr;
    for (const CrossCover &C : X.partners[real])
        if (C.d == d) return &C;
    fail(h, OVQE_ERR_INVALID, "the planned sum has no terms for this rank difference (ovqe_xsum_partners)");
    return nullptr;
}

// sigma = H psi on real amplitudes: the d = 0 groups as one more cover, the shard being its own "partner" and its one chunk
// (m = n_local: no x bits above the chunk, so one class / no displacement above it), built at the first real apply
int xsum_build_local(ovqe_handle h, CrossSum &X) {
    if (X.local_built) return OVQE_OK;
    X.local_cover.d = 0;
    int rc = build_cross_cover(h, X.local_cover, X.raw_local, h->n_local, true);
    if (rc) return rc;
    X.local_built = true;
    return OVQE_OK;
}

// real storage holds sigma only when the sum maps real vectors to real vectors
int xsum_real_apply_ok(ovqe_handle h, const CrossSum &X, const char *who, const void *out_dev) {
    if (!X.real_map)
        return fail(h, OVQE_ERR_STATE, std::string(who) + ": under real_state sigma = H psi needs a real-symmetric sum (every string an even number of Y, "
                                       "every coefficient real); this one would leave the real vectors: clear real_state and widen the buffers");
    const char *s0 = (const char *)h->state, *o0 = (const char *)out_dev;
    const size_t bytes = (size_t)h->namps * sizeof(double);
    if (o0 < s0 + bytes && s0 < o0 + bytes)
        return fail(h, OVQE_ERR_STATE, std::string(who) + ": out overlaps the state buffer (under real_state both hold 2^n_local doubles, not complex amplitudes)");
    return OVQE_OK;
}

}  // namespace

extern "C" {

int ovqe_xsum_create(ovqe_handle h, int64_t T, const uint64_t *x, const uint64_t *z, const double *coeff_re, const double *coeff_im,
                     int chunk_bits, int32_t *id) try {
    OVQE_ENTER(h);
    if (!h || !id || T < 0 || (T && (!x || !z || !coeff_re))) return OVQE_ERR_INVALID;
    if (chunk_bits < 1 || chunk_bits > h->n_local) return fail(h, OVQE_ERR_INVALID, "chunk_bits must lie in 1 .. n_local");
    const uint64_t lmask = local_mask(h);
    const int ntot = h->n_local + h->n_global;
    const uint64_t allmask = ntot >= 64 ? ~0ull : ((1ull << ntot) - 1ull);
    std::unique_ptr<CrossSum, void (*)(CrossSum *)> X(new CrossSum(), free_cross_sum);
    X->chunk_bits = chunk_bits;
    X->hermitian = true;
    std::vector<uint64_t> lx, lz;
    std::vector<double> lr, li;
    std::map<uint64_t, std::map<uint64_t, CrossRawGroup>> remote;   // d -> local x -> group (ascending: the same plan on every rank)
    std::map<uint64_t, CrossRawGroup> local_raw;                    // the d = 0 groups once more, for sigma = H psi on real amplitudes
    X->real_map = true;
    for (int64_t t = 0; t < T; ++t) {
        if ((x[t] | z[t]) & ~allmask) return fail(h, OVQE_ERR_INVALID, "Pauli mask has bits beyond the register");
        const double a = coeff_re[t], b = coeff_im ? coeff_im[t] : 0.0;
        if (b != 0.0) X->hermitian = false;
        if (b != 0.0 || (__builtin_popcountll(x[t] & z[t]) & 1)) X->real_map = false;
        const uint64_t d = x[t] >> h->n_local;
        HTerm ht;
        ht.z = z[t];
        switch (__builtin_popcountll(x[t] & z[t]) & 3) {  // (a + ib) * i^ny
        case 0: ht.cr = a; ht.ci = b; break;
        case 1: ht.cr = -b; ht.ci = a; break;
        case 2: ht.cr = -a; ht.ci = -b; break;
        default: ht.cr = b; ht.ci = -a; break;
        }
        if (d == 0) {
            lx.push_back(x[t]);
            lz.push_back(z[t]);
            lr.push_back(a);
            li.push_back(b);
            CrossRawGroup &g = local_raw[x[t]];
            g.x = x[t];
            g.terms.push_back(ht);
            continue;
        }
        CrossRawGroup &g = remote[d][x[t] & lmask];
        g.x = x[t] & lmask;
        g.terms.push_back(ht);
    }
    if (!lx.empty()) {
        HamDev &H = X->local;
        int rc = build_groups(h, (int64_t)lx.size(), lx.data(), lz.data(), lr.data(), X->hermitian ? nullptr : li.data(), false, H.groups, H.terms);
        if (!rc) rc = upload(h, H.d_groups, H.groups.data(), H.groups.size() * sizeof(HGroup));
        if (!rc) rc = upload(h, H.d_terms, H.terms.data(), H.terms.size() * sizeof(HTerm));
        if (rc) return rc;
        H.set = true;
        H.tile_bits = -1;
        H.version = ++h->ham_versions;
        X->has_local = true;
    }
    for (auto &g : local_raw) X->raw_local.push_back(std::move(g.second));
    for (auto &kv : remote) {
        std::vector<CrossRawGroup> groups;
        for (auto &g : kv.second) groups.push_back(std::move(g.second));
        X->raw.emplace_back(kv.first, std::move(groups));
    }
    X->part_slots = 1;
    int rc = ensure(h, X->d_part, sizeof(double2));
    if (rc) return rc;
    HIPC(h, hipMemsetAsync(X->d_part.p, 0, sizeof(double2), h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    rc = xsum_build(h, *X, h->opt_real_state ? 1 : 0);
    if (rc) return rc;
    int32_t slot = -1;
    for (size_t k = 0; k < h->xsums.size(); ++k)
        if (!h->xsums[k]) slot = (int32_t)k;
    if (slot < 0) {
        h->xsums.push_back(nullptr);
        slot = (int32_t)h->xsums.size() - 1;
    }
    h->xsums[slot] = X.release();
    *id = slot;
    return OVQE_OK;
} OVQE_CATCH(h)

int ovqe_xsum_destroy(ovqe_handle h, int32_t id) try {
    OVQE_ENTER(h);
    CrossSum *X = xsum_of(h, id);
    if (!X) return OVQE_ERR_INVALID;
    HIPC(h, hipStreamSynchronize(h->stream));
    free_cross_sum(X);
    h->xsums[id] = nullptr;
    return OVQE_OK;
} OVQE_CATCH(h)

int ovqe_xsum_partners(ovqe_handle h, int32_t id, int64_t capacity, uint64_t *d, int64_t *passes, int64_t *count) try {
    OVQE_ENTER(h);
    CrossSum *X = xsum_of(h, id);
    if (!X || !count || capacity < 0) return OVQE_ERR_INVALID;
    const int f = h->opt_real_state ? 1 : 0;
    int rc = xsum_build(h, *X, f);
    if (rc) return rc;
    *count = (int64_t)X->partners[f].size();
    for (int64_t k = 0; k < std::min<int64_t>(capacity, *count); ++k) {
        if (d) d[k] = X->partners[f][k].d;
        if (passes) passes[k] = X->partners[f][k].small ? (int64_t)X->partners[f][k].class_h.size() : (int64_t)X->partners[f][k].passes.size();
    }
    return OVQE_OK;
} OVQE_CATCH(h)

int ovqe_xsum_info(ovqe_handle h, int32_t id, int64_t *info, int count) try {
    OVQE_ENTER(h);
    CrossSum *X = xsum_of(h, id);
    if (!X || !info || count < 0) return OVQE_ERR_INVALID;
    int64_t rg = 0, rt = 0, rp = 0, small = 0, M = 0;
    const int f = h->opt_real_state ? 1 : 0;
    int rc = xsum_build(h, *X, f);
    if (rc) return rc;
    for (const CrossCover &C : X->partners[f]) {
        rg += C.ngroups;
        rt += C.nterms;
        rp += C.small ? (int64_t)C.class_h.size() : (int64_t)C.passes.size();
        small |= C.small ? 1 : 0;
        M = std::max<int64_t>(M, C.M);
    }
    const int64_t v[10] = {(int64_t)X->local.groups.size(), (int64_t)X->local.terms.size(), (int64_t)X->local.tsweeps.size(), (int64_t)X->local.n_rest,
                           (int64_t)X->partners[f].size(), rg, rt, rp, M, small};
    for (int k = 0; k < std::min(count, 10); ++k) info[k] = v[k];
    return OVQE_OK;
} OVQE_CATCH(h)

int ovqe_xsum_expect_local(ovqe_handle h, int32_t id, double *out) try {
    OVQE_ENTER(h);
    CrossSum *X = xsum_of(h, id);
    if (!X || !out) return OVQE_ERR_INVALID;
    if (!X->hermitian) return fail(h, OVQE_ERR_INVALID, "expectation value of a sum with complex coefficients");
    *out = 0.0;
    if (!X->has_local) return OVQE_OK;
    HamDev &H = X->local;
    double2 res = make_double2(0.0, 0.0);
    bool tiled = false;
    const bool real = h->opt_real_state != 0;
    int rc = run_expectation_tiled(h, H, &res, &tiled, real);
    if (!rc && !tiled && real) {   // registers too small for the cover: the pair-trick kernel on doubles
        const int nb = reduce_blocks(h->namps);
        rc = ensure(h, h->d_partials, (size_t)nb * sizeof(double2));
        if (!rc) rc = ensure(h, h->d_result, 64 * sizeof(double2));
        if (rc) return rc;
        hipLaunchKernelGGL(k_expect_pairs_real, dim3(nb), dim3(256), 0, h->stream, (const double *)h->state, h->namps, (const HGroup *)H.d_groups.p, 0,
                           (int)H.groups.size(), (const HTerm *)H.d_terms.p, (double2 *)h->d_partials.p);
        hipLaunchKernelGGL(k_reduce, dim3(1), dim3(256), 0, h->stream, (const double2 *)h->d_partials.p, (int64_t)nb, (double2 *)h->d_result.p, 0);
        HIPC(h, hipGetLastError());
        HIPC(h, hipMemcpyAsync(h->h_result, h->d_result.p, sizeof(double2), hipMemcpyDeviceToHost, h->stream));
        HIPC(h, hipStreamSynchronize(h->stream));
        res = h->h_result[0];
    } else if (!rc && !tiled) {
        rc = run_bilinear(h, h->state, h->state, H.groups, (const HGroup *)H.d_groups.p, (const HTerm *)H.d_terms.p, &res, true);
    }
    *out = res.x;
    return rc;
} OVQE_CATCH(h)

int ovqe_xsum_expect_remote(ovqe_handle h, int32_t id, uint64_t d, uint64_t chunk, const void *ket_chunk) try {
    OVQE_ENTER(h);
    CrossSum *X = xsum_of(h, id);
    if (!X || !ket_chunk) return OVQE_ERR_INVALID;
    const bool real = h->opt_real_state != 0;
    const CrossCover *C = xsum_partner(h, *X, d, chunk, real ? 1 : 0);
    if (!C) return OVQE_ERR_INVALID;
    h->last_passes = C->small ? (int64_t)C->class_h.size() : (int64_t)C->passes.size();
    h->last_pass_bytes = (int64_t)((real ? 16.0 : 32.0) * (double)(1ull << X->chunk_bits) * (double)h->last_passes);
    if (real) return run_cross_chunk_real<true>(h, *X, *C, X->chunk_bits, chunk, (const double *)ket_chunk, (double *)h->state);
    return run_cross_chunk<true>(h, *X, *C, chunk, (const amp_t *)ket_chunk, h->state);
} OVQE_CATCH(h)

int ovqe_xsum_expect_finish(ovqe_handle h, int32_t id, double *out_re_im) try {
    OVQE_ENTER(h);
    CrossSum *X = xsum_of(h, id);
    if (!X || !out_re_im) return OVQE_ERR_INVALID;
    int rc = ensure(h, h->d_result, 64 * sizeof(double2));
    if (rc) return rc;
    hipLaunchKernelGGL(k_reduce, dim3(1), dim3(256), 0, h->stream, (const double2 *)X->d_part.p, (int64_t)X->part_slots, (double2 *)h->d_result.p, 0);
    HIPC(h, hipGetLastError());
    HIPC(h, hipMemcpyAsync(h->h_result, h->d_result.p, sizeof(double2), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipMemsetAsync(X->d_part.p, 0, X->part_slots * sizeof(double2), h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    out_re_im[0] = h->h_result[0].x;
    out_re_im[1] = h->h_result[0].y;
    return OVQE_OK;
} OVQE_CATCH(h)

int ovqe_xsum_apply_local(ovqe_handle h, int32_t id, void *out_dev, double ident) try {
    OVQE_ENTER(h);
    CrossSum *X = xsum_of(h, id);
    if (!X || !out_dev) return OVQE_ERR_INVALID;
    if (h->opt_real_state) {   // 2^n_local doubles: out = ident * psi, then the d = 0 cover with the shard as its own ket chunk
        int rc = xsum_real_apply_ok(h, *X, "ovqe_xsum_apply_local", out_dev);
        if (!rc && X->has_local) rc = xsum_build_local(h, *X);
        if (rc) return rc;
        const uint64_t nel = std::max<uint64_t>(h->namps >> 1, 1);   // (the doubles as double2 elements, as ovqe_norm2 reads them)
        hipLaunchKernelGGL(k_axpy_real, dim3(reduce_blocks(nel)), dim3(256), 0, h->stream, (amp_t *)out_dev, (const amp_t *)h->state, ident, nel, 1);
        HIPC(h, hipGetLastError());
        if (!X->has_local) return OVQE_OK;
        const CrossCover &C = X->local_cover;
        h->last_passes = C.small ? (int64_t)C.class_h.size() : (int64_t)C.passes.size();
        h->last_pass_bytes = (int64_t)(24.0 * (double)h->namps * (double)h->last_passes);   // ket read, out read and written
        return run_cross_chunk_real<false>(h, *X, C, h->n_local, 0, (const double *)h->state, (double *)out_dev);
    }
    if (out_dev == (void *)h->state) return fail(h, OVQE_ERR_INVALID, "ovqe_xsum_apply_local: out must differ from the state");
    if (!X->has_local) {   // out = ident * psi
        hipLaunchKernelGGL(k_apply_sum, dim3(reduce_blocks(h->namps)), dim3(256), 0, h->stream, (amp_t *)out_dev, (const amp_t *)h->state,
                           (amp_t *)nullptr, h->namps, h->base, (const HGroup *)nullptr, 0, (const HTerm *)nullptr, 1.0, 0.0, ident, 0.0);
        HIPC(h, hipGetLastError());
        return OVQE_OK;
    }
    return apply_hamiltonian(h, (amp_t *)out_dev, h->state, ident, nullptr, 0, &X->local);
} OVQE_CATCH(h)

int ovqe_xsum_apply_remote(ovqe_handle h, int32_t id, uint64_t d, uint64_t chunk, const void *ket_chunk, void *out_dev) try {
    OVQE_ENTER(h);
    CrossSum *X = xsum_of(h, id);
    if (!X || !ket_chunk || !out_dev) return OVQE_ERR_INVALID;
    if (h->opt_real_state) {
        if (int rc = xsum_real_apply_ok(h, *X, "ovqe_xsum_apply_remote", out_dev)) return rc;
        const CrossCover *C = xsum_partner(h, *X, d, chunk, 1);
        if (!C) return OVQE_ERR_INVALID;
        h->last_passes = C->small ? (int64_t)C->class_h.size() : (int64_t)C->passes.size();
        h->last_pass_bytes = (int64_t)(24.0 * (double)(1ull << X->chunk_bits) * (double)h->last_passes);
        return run_cross_chunk_real<false>(h, *X, *C, X->chunk_bits, chunk, (const double *)ket_chunk, (double *)out_dev);
    }
    const CrossCover *C = xsum_partner(h, *X, d, chunk, 0);
    if (!C) return OVQE_ERR_INVALID;
    return run_cross_chunk<false>(h, *X, *C, chunk, (const amp_t *)ket_chunk, (amp_t *)out_dev);
} OVQE_CATCH(h)

}  // extern "C"
