// cross_host.inc — planned Pauli sums on one shard of the partitioned register: the ovqe_xsum_* entry points (planner:
// sv_cross_host.hpp; kernels: sv_cross.hpp; the multi-rank protocol above them: openvqe_amd/distributed.py).  Included at the end of
// ovqe_sv.hip.
//
// Masks arrive in the PHYSICAL index-bit space of the whole register (n_local + n_global bits).  A term's x part on the rank bits,
// d = x >> n_local, names the partner shard (rank ^ d) its ket amplitudes live in; d = 0 terms act inside the shard.  The plan is
// made once per (Hamiltonian, permutation) — SURVEY.md section 8e: the same Hamiltonian is evaluated at every optimiser step
// (ref:openvqe/ucc_family/get_energy_ucc.py:46-48) and applied at every ADAPT macro-iteration
// (ref:openvqe/adapt/fermionic_adapt_vqe.py:114) — so an evaluation uploads nothing and synchronises once.

namespace {

// a tile pass of cover D over one chunk: KT / KF = the kernel with and without non-temporal loads (shards of ntl_from qubits and more)
template <auto KT, auto KF, class T>
int launch_tile_cross(ovqe_handle h, const CrossCoverDev &D, const TilePass &ps, size_t smem, int ntl_from, const T *ket, T *other,
                      uint64_t ket_gbase, uint64_t chunk_off, unsigned grid, double2 *partials) {
    if (int rc = lds_opt_in<KT, KF>(h, smem)) return rc;
    hipLaunchKernelGGL(h->n_local >= ntl_from ? KT : KF, dim3(grid), dim3(1 << TILE_EXPECT_LOG_NT), smem, h->stream, ket, other, ket_gbase,
                       chunk_off, ps, (const ExChunkT *)D.d_achunks.p, (const ExAGroupT *)D.d_agroups.p, (const ExTermT *)D.d_aterms.p, partials);
    HIPC(h, hipGetLastError());
    return OVQE_OK;
}
template <int M, bool DOT, class... A>
int launch_tile_cross_complex(ovqe_handle h, const CrossCoverDev &D, const TilePass &ps, A... args) {
    constexpr int NT = 1 << TILE_EXPECT_LOG_NT;
    return launch_tile_cross<&k_tile_cross<M, NT, true, DOT>, &k_tile_cross<M, NT, false, DOT>>(
        h, D, ps, tile_apply_lds<M>(sizeof(double2), NT / 64).bytes, 25, args...);
}
template <int M, bool DOT, class... A>
int launch_tile_cross_real(ovqe_handle h, const CrossCoverDev &D, const TilePass &ps, A... args) {
    constexpr int NT = 1 << TILE_EXPECT_LOG_NT;
    return launch_tile_cross<&k_tile_cross_real<M, NT, true, DOT>, &k_tile_cross_real<M, NT, false, DOT>>(
        h, D, ps, tile_apply_lds<M>(sizeof(double), NT / 64).bytes, 26, args...);
}

// the passes of cover C (real flavour) over one chunk of 2^m doubles; DOT: partials += other . (H_d ket), else other += H_d ket.
// A partner's cover takes the received chunks (m = the plan's chunk_bits); the d = 0 cover of sigma = H psi takes the shard itself
// as its one chunk (m = n_local, xsum_build_local).
template <bool DOT>
int run_cross_chunk_real(ovqe_handle h, CrossSum &X, const CrossCoverDev &D, int m, uint64_t chunk, const double *ket, double *other) {
    const cross::Cover &C = D.c;
    const uint64_t csize = 1ull << m;
    const uint64_t ket_gbase = ((h->shard ^ C.d) << h->n_local) | (chunk << m);
    double2 *partials = (double2 *)X.d_part.p;
    if (C.small) {
        const int nb = (int)std::min<uint64_t>(DOT ? X.part_slots : 2048, std::max<uint64_t>(1, (csize + 255) / 256));
        for (size_t k = 0; k < C.class_h.size(); ++k)
            hipLaunchKernelGGL((k_cross_small_real<DOT>), dim3(nb), dim3(256), 0, h->stream, ket, other + ((chunk ^ C.class_h[k]) << m), csize,
                               ket_gbase, (const HGroup *)D.d_groups.p, C.class_groups[k].first, C.class_groups[k].second,
                               (const HTerm *)D.d_terms.p, partials);
        HIPC(h, hipGetLastError());
        return OVQE_OK;
    }
    const unsigned grid = (unsigned)(csize >> C.M);
    for (const TilePass &ps : C.passes) {
        int rc;
        switch (C.M) {
        case 11: rc = launch_tile_cross_real<11, DOT>(h, D, ps, ket, other, ket_gbase, chunk << m, grid, partials); break;
        case 12: rc = launch_tile_cross_real<12, DOT>(h, D, ps, ket, other, ket_gbase, chunk << m, grid, partials); break;
        default: rc = launch_tile_cross_real<13, DOT>(h, D, ps, ket, other, ket_gbase, chunk << m, grid, partials); break;
        }
        if (rc) return rc;
    }
    return OVQE_OK;
}

// every pass of partner cover C over one received chunk; DOT: partials += conj(other) . (H_d ket), else other += H_d ket
template <bool DOT>
int run_cross_chunk(ovqe_handle h, CrossSum &X, const CrossCoverDev &D, uint64_t chunk, const amp_t *ket, amp_t *other) {
    const cross::Cover &C = D.c;
    const int m = X.chunk_bits;
    const uint64_t csize = 1ull << m;
    const uint64_t ket_gbase = ((h->shard ^ C.d) << h->n_local) | (chunk << m);
    double2 *partials = (double2 *)X.d_part.p;
    if (C.small) {
        const int nb = (int)std::min<uint64_t>(X.part_slots, std::max<uint64_t>(1, (csize + 255) / 256));
        for (size_t k = 0; k < C.class_h.size(); ++k) {
            amp_t *oc = other + ((chunk ^ C.class_h[k]) << m);
            hipLaunchKernelGGL((k_cross_small<DOT>), dim3(nb), dim3(256), 0, h->stream, ket, oc, csize, ket_gbase, (const HGroup *)D.d_groups.p,
                               C.class_groups[k].first, C.class_groups[k].second, (const HTerm *)D.d_terms.p, partials);
        }
        HIPC(h, hipGetLastError());
        return OVQE_OK;
    }
    const unsigned grid = (unsigned)(csize >> C.M);
    for (const TilePass &ps : C.passes) {
        int rc;
        switch (C.M) {
        case 10: rc = launch_tile_cross_complex<10, DOT>(h, D, ps, ket, other, ket_gbase, chunk << m, grid, partials); break;
        case 11: rc = launch_tile_cross_complex<11, DOT>(h, D, ps, ket, other, ket_gbase, chunk << m, grid, partials); break;
        default: rc = launch_tile_cross_complex<12, DOT>(h, D, ps, ket, other, ket_gbase, chunk << m, grid, partials); break;
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

// the cover of one partner's groups (sv_cross_host.hpp), on the device.  Between real vectors the terms with an imaginary folded
// coefficient contribute nothing and are dropped (the pool cover, which needs Im v_k, keeps them)
int build_cross_cover(ovqe_handle h, CrossCoverDev &D, const std::vector<cross::RawGroup> &groups, int m, bool real) {
    cross::Cover &C = D.c;
    if (!cross::build_cover(C, groups, m, real, real)) return fail(h, OVQE_ERR_INVALID, "internal: cross-shard cover made no progress");
    if (C.small) {
        int rc = upload(h, D.d_groups, C.groups.data(), C.groups.size() * sizeof(HGroup));
        if (!rc) rc = upload(h, D.d_terms, C.terms.data(), C.terms.size() * sizeof(HTerm));
        return rc;
    }
    int rc = upload(h, D.d_achunks, C.achunks.data(), C.achunks.size() * sizeof(ExChunkT));
    if (!rc) rc = upload(h, D.d_agroups, C.agroups.data(), C.agroups.size() * sizeof(ExAGroupT));
    if (!rc) rc = upload(h, D.d_aterms, C.aterms.data(), C.aterms.size() * sizeof(ExTermT));
    return rc;
}

// the pass lists of every partner for complex (0) or real (1) amplitudes, built at the first use of that flavour
int xsum_build(ovqe_handle h, CrossSum &X, int real) {
    if (X.built[real]) return OVQE_OK;
    size_t slots = X.part_slots;
    X.partners[real].clear();
    X.partners[real].reserve(X.raw.size());
    for (const auto &kv : X.raw) {
        X.partners[real].emplace_back();
        CrossCoverDev &D = X.partners[real].back();
        const cross::Cover &C = D.c;
        D.c.d = kv.first;
        int rc = build_cross_cover(h, D, kv.second, X.chunk_bits, real != 0);
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

const CrossCoverDev *xsum_partner(ovqe_handle h, CrossSum &X, uint64_t d, uint64_t chunk, int real) {
    if (chunk >> (h->n_local - X.chunk_bits)) {
        fail(h, OVQE_ERR_INVALID, "chunk index beyond the shard");
        return nullptr;
    }
    if (xsum_build(h, X, real)) return nullptr;
    for (const CrossCoverDev &D : X.partners[real])
        if (D.c.d == d) return &D;
    fail(h, OVQE_ERR_INVALID, "the planned sum has no terms for this rank difference (ovqe_xsum_partners)");
    return nullptr;
}

// sigma = H psi on real amplitudes: the d = 0 groups as one more cover, the shard being its own "partner" and its one chunk
// (m = n_local: no x bits above the chunk, so one class / no displacement above it), built at the first real apply
int xsum_build_local(ovqe_handle h, CrossSum &X) {
    if (X.local_built) return OVQE_OK;
    X.local_cover.c.d = 0;
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
    std::map<uint64_t, std::map<uint64_t, cross::RawGroup>> remote;   // d -> local x -> group (ascending: the same plan on every rank)
    std::map<uint64_t, cross::RawGroup> local_raw;                    // the d = 0 groups once more, for sigma = H psi on real amplitudes
    X->real_map = true;
    for (int64_t t = 0; t < T; ++t) {
        if ((x[t] | z[t]) & ~allmask) return fail(h, OVQE_ERR_INVALID, "Pauli mask has bits beyond the register");
        const double a = coeff_re[t], b = coeff_im ? coeff_im[t] : 0.0;
        if (b != 0.0) X->hermitian = false;
        if (b != 0.0 || (__builtin_popcountll(x[t] & z[t]) & 1)) X->real_map = false;
        const uint64_t d = x[t] >> h->n_local;
        HTerm ht;
        ht.z = z[t];
        fold_iny(a, b, __builtin_popcountll(x[t] & z[t]), ht.cr, ht.ci);
        if (d == 0) {
            lx.push_back(x[t]);
            lz.push_back(z[t]);
            lr.push_back(a);
            li.push_back(b);
            cross::RawGroup &g = local_raw[x[t]];
            g.x = x[t];
            g.terms.push_back(ht);
            continue;
        }
        cross::RawGroup &g = remote[d][x[t] & lmask];
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
        std::vector<cross::RawGroup> groups;
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
        if (d) d[k] = X->partners[f][k].c.d;
        if (passes) passes[k] = X->partners[f][k].c.n_passes();
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
    for (const CrossCoverDev &D : X->partners[f]) {
        const cross::Cover &C = D.c;
        rg += C.ngroups;
        rt += C.nterms;
        rp += C.n_passes();
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
        rc = reduce_to_host(h, h->d_partials.p, nb, &res);
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
    const CrossCoverDev *C = xsum_partner(h, *X, d, chunk, real ? 1 : 0);
    if (!C) return OVQE_ERR_INVALID;
    h->last_passes = C->c.n_passes();
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
        const CrossCoverDev &C = X->local_cover;
        h->last_passes = C.c.n_passes();
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
        const CrossCoverDev *C = xsum_partner(h, *X, d, chunk, 1);
        if (!C) return OVQE_ERR_INVALID;
        h->last_passes = C->c.n_passes();
        h->last_pass_bytes = (int64_t)(24.0 * (double)(1ull << X->chunk_bits) * (double)h->last_passes);
        return run_cross_chunk_real<false>(h, *X, *C, X->chunk_bits, chunk, (const double *)ket_chunk, (double *)out_dev);
    }
    const CrossCoverDev *C = xsum_partner(h, *X, d, chunk, 0);
    if (!C) return OVQE_ERR_INVALID;
    return run_cross_chunk<false>(h, *X, *C, chunk, (const amp_t *)ket_chunk, (amp_t *)out_dev);
} OVQE_CATCH(h)

}  // extern "C"
