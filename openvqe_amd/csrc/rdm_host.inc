// rdm_host.inc — handle section of the one- and two-particle density matrices (plan: sv_rdm_host.hpp; kernels: sv_rdm.hpp; entry
// points: abi_rdm.inc).  Included by ovqe_sv.hip inside its anonymous namespace.
//
// One call: census of the state (bitmap of the support, non-zero count, real / complex), one or two down-shadows, the ascending list
// of the shadow's bits (the rows), then per workspace chunk the rows kernel and the Gram kernel, and the reduction of the slabs.
// Everything runs on the handle's stream in order; the host waits three times (census, row count, result).

struct RdmDev {
    DevBuf d_bitmap[2], d_census, d_counts, d_start, d_scan_temp, d_rows, d_cols, d_ws, d_slabs, d_out;
    std::vector<rdm::ColEntry> cols;
    int cols_n = 0, cols_order = 0;           // what `cols` / d_cols hold
    std::vector<hipEvent_t> ev;               // phase boundaries of the last call
    int64_t info[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
};

void free_rdm(RdmDev *R) {
    if (!R) return;
    for (DevBuf *b : {&R->d_bitmap[0], &R->d_bitmap[1], &R->d_census, &R->d_counts, &R->d_start, &R->d_scan_temp, &R->d_rows, &R->d_cols,
                      &R->d_ws, &R->d_slabs, &R->d_out})
        if (b->p) (void)hipFree(b->p);
    for (hipEvent_t e : R->ev)
        if (e) (void)hipEventDestroy(e);
    delete R;
}

int rdm_event(ovqe_handle h, RdmDev &R, size_t k) {
    while (R.ev.size() <= k) {
        hipEvent_t e = nullptr;
        HIPC(h, hipEventCreate(&e));
        R.ev.push_back(e);
    }
    HIPC(h, hipEventRecord(R.ev[k], h->stream));
    return OVQE_OK;
}

int run_rdm(ovqe_handle h, int order, double *out) {
    const int n = h->n_local;
    if (!h->rdm) h->rdm = new RdmDev();
    RdmDev &R = *h->rdm;
    std::fill(R.info, R.info + 12, 0);
    handle_num_cus(h);
    const int64_t W = rdm::width(n, order);
    const uint64_t nwords = rdm::bitmap_words(n);
    int rc = OVQE_OK;
    // ---- census
    const int cb = (int)std::min<uint64_t>(1024, (nwords + 3) / 4);
    for (int k = 0; k < 2; ++k)
        if ((rc = ensure(h, R.d_bitmap[k], nwords * sizeof(uint64_t)))) return rc;
    if ((rc = ensure(h, R.d_census, 1024 * sizeof(ulonglong2)))) return rc;
    if ((rc = rdm_event(h, R, 0))) return rc;
    hipLaunchKernelGGL(k_rdm_census, dim3(cb), dim3(256), 0, h->stream, (const amp_t *)h->state, h->namps, nwords, (uint64_t *)R.d_bitmap[0].p,
                       (ulonglong2 *)R.d_census.p);
    HIPC(h, hipGetLastError());
    std::vector<ulonglong2> census(cb);
    HIPC(h, hipMemcpyAsync(census.data(), R.d_census.p, (size_t)cb * sizeof(ulonglong2), hipMemcpyDeviceToHost, h->stream));
    // ---- down-shadows: B0 -> B1 (-> B2), ping-pong
    const unsigned wb = (unsigned)((nwords + 255) / 256);
    int cur = 0;
    for (int k = 0; k < order; ++k, cur ^= 1) {
        hipLaunchKernelGGL(k_rdm_shadow, dim3(wb), dim3(256), 0, h->stream, (const uint64_t *)R.d_bitmap[cur].p, (uint64_t *)R.d_bitmap[cur ^ 1].p,
                           nwords, n);
        HIPC(h, hipGetLastError());
    }
    const uint64_t *shadow = (const uint64_t *)R.d_bitmap[cur].p;
    // ---- row list: popcounts, their prefix sums, the set bits in ascending order
    if ((rc = ensure(h, R.d_counts, (nwords + 1) * sizeof(uint64_t)))) return rc;
    if ((rc = ensure(h, R.d_start, (nwords + 1) * sizeof(uint64_t)))) return rc;
    hipLaunchKernelGGL(k_rdm_popc, dim3((unsigned)((nwords + 256) / 256)), dim3(256), 0, h->stream, shadow, nwords, (uint64_t *)R.d_counts.p);
    HIPC(h, hipGetLastError());
    {
        size_t tb = 0;
        hipError_t e = hipcub::DeviceScan::ExclusiveSum(nullptr, tb, (const uint64_t *)R.d_counts.p, (uint64_t *)R.d_start.p, (int)(nwords + 1), h->stream);
        if (e != hipSuccess) return fail(h, OVQE_ERR_HIP, std::string("scan (size query): ") + hipGetErrorString(e));
        if ((rc = ensure(h, R.d_scan_temp, tb))) return rc;
        tb = R.d_scan_temp.cap;
        e = hipcub::DeviceScan::ExclusiveSum(R.d_scan_temp.p, tb, (const uint64_t *)R.d_counts.p, (uint64_t *)R.d_start.p, (int)(nwords + 1), h->stream);
        if (e != hipSuccess) return fail(h, OVQE_ERR_HIP, std::string("scan: ") + hipGetErrorString(e));
    }
    uint64_t nrows_u = 0;
    HIPC(h, hipMemcpyAsync(&nrows_u, (const uint64_t *)R.d_start.p + nwords, sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    uint64_t nnz = 0, any_im = 0;
    for (const ulonglong2 &c : census) {
        nnz += c.x;
        any_im |= c.y;
    }
    const bool real = any_im == 0;
    const int64_t nrows = (int64_t)nrows_u;
    const rdm::Schedule S = rdm::plan(n, order, real, nrows, h->opt_rdm_workspace_mb, h->num_cus);
    if ((rc = ensure(h, R.d_rows, (size_t)std::max<int64_t>(nrows, 1) * sizeof(uint64_t)))) return rc;
    hipLaunchKernelGGL(k_rdm_list, dim3(wb), dim3(256), 0, h->stream, shadow, nwords, (const uint64_t *)R.d_start.p, (uint64_t *)R.d_rows.p);
    HIPC(h, hipGetLastError());
    if (R.cols_n != n || R.cols_order != order) {
        rdm::build_columns(n, order, R.cols);
        if ((rc = upload(h, R.d_cols, R.cols.data(), R.cols.size() * sizeof(rdm::ColEntry)))) return rc;
        R.cols_n = n;
        R.cols_order = order;
    }
    // ---- rows and Gram, chunk by chunk
    const size_t slab_bytes = S.slab_elems * S.elem_bytes;
    if ((rc = ensure(h, R.d_ws, S.workspace_bytes))) return rc;
    if ((rc = ensure(h, R.d_slabs, slab_bytes))) return rc;
    if ((rc = ensure(h, R.d_out, (size_t)W * W * sizeof(double2)))) return rc;
    HIPC(h, hipMemsetAsync(R.d_slabs.p, 0, slab_bytes, h->stream));
    const bool timed = S.nchunks <= rdm::TIMED_CHUNKS_MAX;
    if ((rc = rdm_event(h, R, 1))) return rc;
    constexpr RdmGramLds L = rdm_gram_lds();
    for (int64_t c = 0; c < S.nchunks; ++c) {
        const int64_t row0 = c * S.chunk_rows, cr = std::min(S.chunk_rows, nrows - row0);
        const unsigned rb = (unsigned)std::min<uint64_t>(((uint64_t)cr * S.wpad + 255) / 256, (uint64_t)h->num_cus * 16u);
        const uint64_t *rows = (const uint64_t *)R.d_rows.p + row0;
        const rdm::ColEntry *cols = (const rdm::ColEntry *)R.d_cols.p;
        const unsigned gb = (unsigned)(S.npairs * S.slices);
        if (real) {
            hipLaunchKernelGGL(k_rdm_rows<true>, dim3(rb), dim3(256), 0, h->stream, (const amp_t *)h->state, rows, cr, cols, W, S.wpad, R.d_ws.p);
            if (timed && (rc = rdm_event(h, R, 2 + 2 * (size_t)c))) return rc;
            hipLaunchKernelGGL(k_rdm_gram<true>, dim3(gb), dim3(rdm::GRAM_THREADS), L.bytes, h->stream, (const void *)R.d_ws.p, cr, S.wpad, S.nblk,
                               S.slices, S.slice_rows, R.d_slabs.p);
        } else {
            hipLaunchKernelGGL(k_rdm_rows<false>, dim3(rb), dim3(256), 0, h->stream, (const amp_t *)h->state, rows, cr, cols, W, S.wpad, R.d_ws.p);
            if (timed && (rc = rdm_event(h, R, 2 + 2 * (size_t)c))) return rc;
            hipLaunchKernelGGL(k_rdm_gram<false>, dim3(gb), dim3(rdm::GRAM_THREADS), L.bytes, h->stream, (const void *)R.d_ws.p, cr, S.wpad, S.nblk,
                               S.slices, S.slice_rows, R.d_slabs.p);
        }
        HIPC(h, hipGetLastError());
        if (timed && (rc = rdm_event(h, R, 3 + 2 * (size_t)c))) return rc;
    }
    // ---- finish
    const size_t ev_fin = timed ? 2 + 2 * (size_t)S.nchunks : 2;
    const unsigned fb = (unsigned)(((uint64_t)W * W + 255) / 256);
    if (real) hipLaunchKernelGGL(k_rdm_finish<true>, dim3(fb), dim3(256), 0, h->stream, (const void *)R.d_slabs.p, W, S.nblk, S.slices, (double2 *)R.d_out.p);
    else hipLaunchKernelGGL(k_rdm_finish<false>, dim3(fb), dim3(256), 0, h->stream, (const void *)R.d_slabs.p, W, S.nblk, S.slices, (double2 *)R.d_out.p);
    HIPC(h, hipGetLastError());
    if ((rc = rdm_event(h, R, ev_fin))) return rc;
    HIPC(h, hipMemcpyAsync(out, R.d_out.p, (size_t)W * W * sizeof(double2), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    // ---- what happened
    R.info[0] = (int64_t)nnz;
    R.info[1] = nrows;
    R.info[2] = S.nchunks;
    R.info[3] = real ? 1 : 0;
    R.info[4] = (int64_t)S.workspace_bytes;
    R.info[5] = S.nchunks;
    R.info[6] = S.npairs;
    R.info[7] = S.slices;
    float ms = 0.f;
    HIPC(h, hipEventElapsedTime(&ms, R.ev[0], R.ev[1]));
    R.info[8] = (int64_t)(1e3 * ms);
    if (timed) {
        double rows_ms = 0.0, gram_ms = 0.0;
        for (int64_t c = 0; c < S.nchunks; ++c) {
            HIPC(h, hipEventElapsedTime(&ms, R.ev[1 + 2 * (size_t)c], R.ev[2 + 2 * (size_t)c]));
            rows_ms += ms;
            HIPC(h, hipEventElapsedTime(&ms, R.ev[2 + 2 * (size_t)c], R.ev[3 + 2 * (size_t)c]));
            gram_ms += ms;
        }
        R.info[9] = (int64_t)(1e3 * rows_ms);
        R.info[10] = (int64_t)(1e3 * gram_ms);
        HIPC(h, hipEventElapsedTime(&ms, R.ev[ev_fin - 1], R.ev[ev_fin]));
        R.info[11] = (int64_t)(1e3 * ms);
    }
    return OVQE_OK;
}
