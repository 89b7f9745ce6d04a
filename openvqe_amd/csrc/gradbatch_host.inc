// gradbatch_host.inc — handle section of the batched exact gradient (geometry: sv_gradbatch_host.hpp; kernel: k_sparse_grad_batch in
// sv_sparse.hpp; entry points: abi_gradbatch.inc).  Included by ovqe_sv.hip inside its anonymous namespace.
//
// Path 1: the handle's compact program as run_sparse_gradient uses it (d_sp_ops, d_sp_pairs, d_rots, d_sp_entries), the whole batch in
// one launch.  Nothing is planned or built here beyond what the single call builds on its first use.  Everything the call allocates is
// this record's: h->d_theta, the mapped I/O slot and sp_forms are not touched.  Path 2 (every other program): abi_gradbatch.inc runs
// the single call's body row by row.

static_assert(gradbatch::LDS_BUDGET == LDS_WG_BUDGET && gradbatch::LDS_CU == LDS_WG_MAX, "sv_gradbatch_host.hpp plans with this file's budgets");

struct GradBatchDev {
    DevBuf d_theta, d_out;   // rows [B * K]; energies [B], then gradients [B * K]
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    int64_t info[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
};

void free_grad_batch(GradBatchDev *D) {
    if (!D) return;
    for (DevBuf *b : {&D->d_theta, &D->d_out})
        if (b->p) (void)hipFree(b->p);
    for (hipEvent_t e : D->ev)
        if (e) (void)hipEventDestroy(e);
    delete D;
}

template <int NW>
int launch_grad_batch(ovqe_handle h, bool stage, unsigned grid, size_t lds, const SparseArgs &A, const double *d_theta, double *d_e, double *d_g) {
    constexpr auto staged = &k_sparse_grad_batch<NW, true>, plain = &k_sparse_grad_batch<NW, false>;
    if (int rc = lds_opt_in<staged, plain>(h, LDS_WG_MAX)) return rc;
    hipLaunchKernelGGL(stage ? staged : plain, dim3(grid), dim3(NW * 64), lds, h->stream, A, d_theta,
                       (const SmallRot *)h->d_rots.p, (const SpOp *)h->d_sp_ops.p, (const uint32_t *)h->d_sp_pairs.p,
                       (const SpEntry *)h->d_sp_entries.p, d_e, d_g);
    HIPC(h, hipGetLastError());
    return OVQE_OK;
}

// *done = false: the program is not eligible for path 1 (nothing was launched, info untouched)
int run_grad_batch(ovqe_handle h, int64_t B, const double *theta, double *energies, double *grads, bool *done) {
    *done = false;
    if (!(h->opt_force_path == 0 || h->opt_force_path == 3) || !h->opt_sparse_grad || h->n_local > 16) return OVQE_OK;
    int rc = OVQE_OK;
    if (!h->sp_tried && (rc = build_sparse_program(h))) return rc;
    if (!h->sp_valid) return OVQE_OK;
    SparseArgs A;
    A.m = h->sp_mp;
    A.mpad = (h->sp_mp + 1) & ~1;
    A.hf = h->sp_hf;
    A.K = h->K;
    A.nops = h->sp_nops;
    A.ntab = (int)h->srots.size();
    A.nent = h->sp_nent;
    A.npairs = (int)h->sp_npairs;
    A.B = B;
    A.constant = h->ham.constant;
    if (!gradbatch::eligible(A)) return OVQE_OK;
    const gradbatch::Plan G = gradbatch::plan(A, B, h->opt_grad_batch_waves, h->opt_grad_batch_workgroups, handle_num_cus(h));
    if (!G.ok) return OVQE_OK;
    if (!h->grad_batch) h->grad_batch = new GradBatchDev();
    GradBatchDev &D = *h->grad_batch;
    if ((rc = ensure_events(h, D.ev, 3))) return rc;
    const size_t K = (size_t)h->K, rows = (size_t)B * K;
    if ((rc = ensure(h, D.d_theta, rows * sizeof(double)))) return rc;
    if ((rc = ensure(h, D.d_out, ((size_t)B + rows) * sizeof(double)))) return rc;
    double *d_e = (double *)D.d_out.p, *d_g = d_e + B;
    HIPC(h, hipEventRecord(D.ev[0], h->stream));
    HIPC(h, hipMemcpyAsync(D.d_theta.p, theta, rows * sizeof(double), hipMemcpyHostToDevice, h->stream));
    const unsigned grid = (unsigned)G.workgroups;
    switch (G.nw) {
    case 1: rc = launch_grad_batch<1>(h, G.stage, grid, G.lds, A, (const double *)D.d_theta.p, d_e, d_g); break;
    case 2: rc = launch_grad_batch<2>(h, G.stage, grid, G.lds, A, (const double *)D.d_theta.p, d_e, d_g); break;
    case 4: rc = launch_grad_batch<4>(h, G.stage, grid, G.lds, A, (const double *)D.d_theta.p, d_e, d_g); break;
    default: rc = launch_grad_batch<8>(h, G.stage, grid, G.lds, A, (const double *)D.d_theta.p, d_e, d_g); break;
    }
    if (rc) return rc;
    HIPC(h, hipEventRecord(D.ev[1], h->stream));
    HIPC(h, hipMemcpyAsync(energies, d_e, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipMemcpyAsync(grads, d_g, rows * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipEventRecord(D.ev[2], h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    const int64_t info[9] = {1, B, (int64_t)K, 1, G.stage ? 1 : 2, G.nw, G.workgroups, (int64_t)G.lds, h->sp_m};
    std::copy(info, info + 9, D.info);
    if ((rc = phases_us(h, D.ev, 2, D.info + 9))) return rc;
    *done = true;
    return OVQE_OK;
}
