// subspace_host.inc — handle section of the subspace-expansion matrices (plan: sv_subspace_host.hpp; kernels: sv_subspace.hpp and the
// census / popcount / list / finish kernels of sv_rdm.hpp; entry points: abi_subspace.inc).  Included by ovqe_sv.hip inside its
// anonymous namespace.
//
// One call: census of the state (bitmap of the support), its image under every distinct x mask of the pool (the rows R), the ascending
// list of R, then the expansion vectors phi_j = O_j psi into an index-major store, sigma_j = H phi_j on R next to them, and the Gram
// blocks of (Phi, Phi) and (Phi, Sigma).  Everything the call allocates is its own: no table of the energy paths is touched and the
// state buffer is only read.  Everything runs on the handle's stream in order; the host waits for the row count and for the result.

struct SubspaceDev {
    DevBuf d_bitmap[2], d_census, d_counts, d_start, d_scan_temp, d_rows, d_dx, d_off, d_xs, d_terms, d_store, d_slabs, d_out;
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    std::vector<double2> host_out;
    int64_t info[20] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
};

void free_subspace(SubspaceDev *Q) {
    if (!Q) return;
    for (DevBuf *b : {&Q->d_bitmap[0], &Q->d_bitmap[1], &Q->d_census, &Q->d_counts, &Q->d_start, &Q->d_scan_temp, &Q->d_rows, &Q->d_dx, &Q->d_off,
                      &Q->d_xs, &Q->d_terms, &Q->d_store, &Q->d_slabs, &Q->d_out})
        if (b->p) (void)hipFree(b->p);
    for (hipEvent_t e : Q->ev)
        if (e) (void)hipEventDestroy(e);
    delete Q;
}

template <bool DENSE>
int launch_sub_sigma(ovqe_handle h, SubspaceDev &Q, const sub::Plan &P, int64_t *launches, int64_t *grid_x) {
    const unsigned gx = (unsigned)std::min<int64_t>(P.sigma_row_tiles, (int64_t)h->num_cus * 32);
    const dim3 grid(gx, (unsigned)P.sigma_col_groups), block(sub::SIGMA_THREADS);
    const HGroup *groups = (const HGroup *)h->ham.d_groups.p;
    const HTerm *terms = (const HTerm *)h->ham.d_terms.p;
    const int ng = (int)h->ham.groups.size();
    v2d *store = (v2d *)Q.d_store.p;
    const uint64_t *rows = (const uint64_t *)Q.d_rows.p, *bitmap = (const uint64_t *)Q.d_bitmap[1].p, *start = (const uint64_t *)Q.d_start.p;
    if (P.sigma_blocks == 1)
        hipLaunchKernelGGL((k_sub_sigma<DENSE, 1>), grid, block, 0, h->stream, store, rows, P.rows, bitmap, start, groups, ng, terms, h->ham.constant, P.nb, P.mb, P.wpad);
    else if (P.sigma_blocks == 2)
        hipLaunchKernelGGL((k_sub_sigma<DENSE, 2>), grid, block, 0, h->stream, store, rows, P.rows, bitmap, start, groups, ng, terms, h->ham.constant, P.nb, P.mb, P.wpad);
    else
        hipLaunchKernelGGL((k_sub_sigma<DENSE, sub::SIGMA_MAX_BLOCKS>), grid, block, 0, h->stream, store, rows, P.rows, bitmap, start, groups, ng, terms, h->ham.constant, P.nb, P.mb, P.wpad);
    HIPC(h, hipGetLastError());
    ++*launches;
    *grid_x = gx;
    return OVQE_OK;
}

// the arguments were checked by the entry point (offsets monotone, masks inside the register)
int run_subspace(ovqe_handle h, int64_t m, const int64_t *offsets, const uint64_t *x, const uint64_t *z, const double *cr, const double *ci,
                 double *h_out, double *s_out) {
    const int n = h->n_local;
    if (!h->subspace) h->subspace = new SubspaceDev();
    SubspaceDev &Q = *h->subspace;
    std::fill(Q.info, Q.info + 20, 0);
    handle_num_cus(h);
    if (int rc = ensure_events(h, Q.ev, 5)) return rc;
    const bool with_h = h_out != nullptr;
    const int64_t T = offsets[m] - offsets[0];
    const uint64_t nwords = rdm::bitmap_words(n);
    int rc = OVQE_OK;
    // ---- the pool on the device: terms in the caller's order with i^ny folded, their x masks, the CSR offsets from 0; the distinct x
    std::vector<HTerm> terms((size_t)std::max<int64_t>(T, 1));
    std::vector<uint64_t> xs((size_t)std::max<int64_t>(T, 1), 0);
    std::vector<int64_t> off((size_t)m + 1);
    for (int64_t k = 0; k <= m; ++k) off[(size_t)k] = offsets[k] - offsets[0];
    for (int64_t t = 0; t < T; ++t) {
        const int64_t s = offsets[0] + t;
        HTerm ht;
        ht.z = z[s];
        fold_iny(cr[s], ci ? ci[s] : 0.0, __builtin_popcountll(x[s] & z[s]), ht.cr, ht.ci);
        terms[(size_t)t] = ht;
        xs[(size_t)t] = x[s];
    }
    const std::vector<uint64_t> dx = sub::distinct_x(xs.data(), T);   // (empty for a pool without terms: no rows)
    if ((rc = upload(h, Q.d_off, off.data(), off.size() * sizeof(int64_t)))) return rc;
    if ((rc = upload(h, Q.d_xs, xs.data(), xs.size() * sizeof(uint64_t)))) return rc;
    if ((rc = upload(h, Q.d_terms, terms.data(), terms.size() * sizeof(HTerm)))) return rc;
    if ((rc = dx.empty() ? ensure(h, Q.d_dx, sizeof(uint64_t)) : upload(h, Q.d_dx, dx.data(), dx.size() * sizeof(uint64_t)))) return rc;
    // ---- rows: census, the support moved by every x, popcounts, their prefix sums, the set bits in ascending order
    const int cb = (int)std::min<uint64_t>(1024, (nwords + 3) / 4);
    for (int k = 0; k < 2; ++k)
        if ((rc = ensure(h, Q.d_bitmap[k], nwords * sizeof(uint64_t)))) return rc;
    if ((rc = ensure(h, Q.d_census, 1024 * sizeof(ulonglong2)))) return rc;
    if ((rc = ensure(h, Q.d_counts, (nwords + 1) * sizeof(uint64_t)))) return rc;
    if ((rc = ensure(h, Q.d_start, (nwords + 1) * sizeof(uint64_t)))) return rc;
    HIPC(h, hipEventRecord(Q.ev[0], h->stream));
    hipLaunchKernelGGL(k_rdm_census, dim3(cb), dim3(256), 0, h->stream, (const amp_t *)h->state, h->namps, nwords, (uint64_t *)Q.d_bitmap[0].p,
                       (ulonglong2 *)Q.d_census.p);
    HIPC(h, hipGetLastError());
    const unsigned wb = (unsigned)((nwords + 255) / 256);
    const uint64_t *R = (const uint64_t *)Q.d_bitmap[1].p;
    hipLaunchKernelGGL(k_sub_shadow, dim3(wb), dim3(256), 0, h->stream, (const uint64_t *)Q.d_bitmap[0].p, (uint64_t *)Q.d_bitmap[1].p, nwords,
                       (const uint64_t *)Q.d_dx.p, (int)dx.size());
    HIPC(h, hipGetLastError());
    hipLaunchKernelGGL(k_rdm_popc, dim3((unsigned)((nwords + 256) / 256)), dim3(256), 0, h->stream, R, nwords, (uint64_t *)Q.d_counts.p);
    HIPC(h, hipGetLastError());
    {
        size_t tb = 0;
        hipError_t e = hipcub::DeviceScan::ExclusiveSum(nullptr, tb, (const uint64_t *)Q.d_counts.p, (uint64_t *)Q.d_start.p, (int)(nwords + 1), h->stream);
        if (e != hipSuccess) return fail(h, OVQE_ERR_HIP, std::string("scan (size query): ") + hipGetErrorString(e));
        if ((rc = ensure(h, Q.d_scan_temp, tb))) return rc;
        tb = Q.d_scan_temp.cap;
        e = hipcub::DeviceScan::ExclusiveSum(Q.d_scan_temp.p, tb, (const uint64_t *)Q.d_counts.p, (uint64_t *)Q.d_start.p, (int)(nwords + 1), h->stream);
        if (e != hipSuccess) return fail(h, OVQE_ERR_HIP, std::string("scan: ") + hipGetErrorString(e));
    }
    uint64_t nrows_u = 0;
    HIPC(h, hipMemcpyAsync(&nrows_u, (const uint64_t *)Q.d_start.p + nwords, sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    const int64_t nrows = (int64_t)nrows_u;
    const bool dense = nrows_u == h->namps;
    const sub::Plan P = sub::plan(nrows, m, with_h, h->num_cus);
    // ---- the store behind its cap
    rc = workspace_cap(h, h->opt_subspace_workspace_mb, P.store_bytes, Q.d_store.cap, Q.d_store.cap >= P.store_bytes, [&](size_t limit) {
        return "ovqe_subspace_matrices: the store needs " + std::to_string(P.store_bytes) + " bytes (" + std::to_string(nrows) + " rows x " +
               std::to_string(P.wpad) + " columns), the cap is " + std::to_string(limit) + " bytes (option subspace_workspace_mb)";
    });
    if (rc) return rc;
    const size_t out_elems = (size_t)m * (size_t)m * (with_h ? 2u : 1u);
    if ((rc = ensure(h, Q.d_rows, (size_t)std::max<int64_t>(nrows, 1) * sizeof(uint64_t)))) return rc;
    if ((rc = ensure(h, Q.d_store, std::max<size_t>(P.store_bytes, 16)))) return rc;
    if ((rc = ensure(h, Q.d_slabs, P.slab_elems * sizeof(double2)))) return rc;
    if ((rc = ensure(h, Q.d_out, out_elems * sizeof(double2)))) return rc;
    if (!dense) {
        hipLaunchKernelGGL(k_rdm_list, dim3(wb), dim3(256), 0, h->stream, R, nwords, (const uint64_t *)Q.d_start.p, (uint64_t *)Q.d_rows.p);
        HIPC(h, hipGetLastError());
    }
    HIPC(h, hipEventRecord(Q.ev[1], h->stream));
    int64_t expand_launches = 0, sigma_launches = 0, gram_launches = 0, expand_grid = 0, sigma_grid = 0;
    // ---- expand: Phi
    if (nrows > 0) {
        const unsigned eb = (unsigned)std::min<uint64_t>(((uint64_t)nrows * (uint64_t)P.mb + 255) / 256, (uint64_t)h->num_cus * 16u);
        if (dense)
            hipLaunchKernelGGL(k_sub_expand<true>, dim3(eb), dim3(256), 0, h->stream, (const amp_t *)h->state, (const uint64_t *)Q.d_rows.p, nrows,
                               (const int64_t *)Q.d_off.p, (const uint64_t *)Q.d_xs.p, (const HTerm *)Q.d_terms.p, m, P.mb, P.wpad, (v2d *)Q.d_store.p);
        else
            hipLaunchKernelGGL(k_sub_expand<false>, dim3(eb), dim3(256), 0, h->stream, (const amp_t *)h->state, (const uint64_t *)Q.d_rows.p, nrows,
                               (const int64_t *)Q.d_off.p, (const uint64_t *)Q.d_xs.p, (const HTerm *)Q.d_terms.p, m, P.mb, P.wpad, (v2d *)Q.d_store.p);
        HIPC(h, hipGetLastError());
        ++expand_launches;
        expand_grid = eb;
    }
    HIPC(h, hipEventRecord(Q.ev[2], h->stream));
    // ---- sigma: H Phi on R, the stored Hamiltonian's x-groups and its constant
    if (with_h && nrows > 0) {
        rc = dense ? launch_sub_sigma<true>(h, Q, P, &sigma_launches, &sigma_grid) : launch_sub_sigma<false>(h, Q, P, &sigma_launches, &sigma_grid);
        if (rc) return rc;
    }
    HIPC(h, hipEventRecord(Q.ev[3], h->stream));
    // ---- Gram blocks and the two finishes: S mirrored from its upper triangle, Phi^H Sigma entry by entry
    constexpr sub::GramLds GL = sub::gram_lds();
    hipLaunchKernelGGL(k_sub_gram, dim3((unsigned)(P.npairs * P.slices)), dim3(rdm::GRAM_THREADS), GL.bytes, h->stream, (const v2d *)Q.d_store.p, nrows,
                       P.wpad, P.nb, P.slices, P.slice_rows, (v2d *)Q.d_slabs.p);
    HIPC(h, hipGetLastError());
    ++gram_launches;
    const unsigned fb = (unsigned)(((uint64_t)m * (uint64_t)m + 255) / 256);
    hipLaunchKernelGGL(k_rdm_finish<false>, dim3(fb), dim3(256), 0, h->stream, (const void *)Q.d_slabs.p, m, P.nb, P.slices, (double2 *)Q.d_out.p);
    HIPC(h, hipGetLastError());
    if (with_h) {
        hipLaunchKernelGGL(k_sub_finish_full, dim3(fb), dim3(256), 0, h->stream, (const v2d *)Q.d_slabs.p, m, P.nb, P.slices,
                           (double2 *)Q.d_out.p + (size_t)m * (size_t)m);
        HIPC(h, hipGetLastError());
    }
    HIPC(h, hipEventRecord(Q.ev[4], h->stream));
    Q.host_out.resize(out_elems);
    HIPC(h, hipMemcpyAsync(Q.host_out.data(), Q.d_out.p, out_elems * sizeof(double2), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    std::memcpy(s_out, Q.host_out.data(), (size_t)m * (size_t)m * sizeof(double2));
    if (with_h) std::memcpy(h_out, Q.host_out.data() + (size_t)m * (size_t)m, (size_t)m * (size_t)m * sizeof(double2));
    // ---- what happened
    Q.info[0] = m;
    Q.info[1] = nrows;
    Q.info[2] = dense ? 1 : 0;
    Q.info[3] = (int64_t)P.store_bytes;
    Q.info[4] = (int64_t)dx.size();
    Q.info[5] = with_h ? (int64_t)h->ham.groups.size() : 0;
    Q.info[6] = expand_launches;
    Q.info[7] = sigma_launches;
    Q.info[8] = gram_launches;
    Q.info[9] = P.npairs;
    if ((rc = phases_us(h, Q.ev, 4, Q.info + 10))) return rc;
    // which path the call took: the Gram slices, the sigma instantiation and its grid (zeros when no sigma kernel ran), the expand grid
    Q.info[14] = P.slices;
    Q.info[15] = P.slice_rows;
    Q.info[16] = sigma_launches ? P.sigma_blocks : 0;
    Q.info[17] = sigma_launches ? P.sigma_col_groups : 0;
    Q.info[18] = sigma_grid;
    Q.info[19] = expand_grid;
    return OVQE_OK;
}
