// spread_host.inc — handle section of the energy spread S = ||(H - omega) psi||^2 with its gradient (geometry and eligibility:
// sv_spread_host.hpp; kernel: k_sparse_spread_batch in sv_sparse.hpp; entry points and the streaming path: abi_spread.inc).  Included
// by ovqe_sv.hip inside its anonymous namespace.
//
// Path 1 is run_grad_batch's — the handle's compact program as it stands, the whole batch in one launch — where three state arrays of
// one wave fit the budget AND the restricted entries are H on the support (h->sp_exact, decided once with the compact program in
// build_sparse_program).  Nothing is planned or built here beyond what the single gradient builds on its first use; everything the
// call allocates is this record's.

struct SpreadDev {
    DevBuf d_theta, d_omega, d_out;   // rows [B * K]; omega [B]; costs [B], energies [B], spreads [B], gradients [B * K]
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    int64_t info[13] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
};

void free_spread(SpreadDev *D) {
    if (!D) return;
    for (DevBuf *b : {&D->d_theta, &D->d_omega, &D->d_out})
        if (b->p) (void)hipFree(b->p);
    for (hipEvent_t e : D->ev)
        if (e) (void)hipEventDestroy(e);
    delete D;
}

SpreadDev &spread_dev(ovqe_handle h) {
    if (!h->spread) h->spread = new SpreadDev();
    return *h->spread;
}

template <int NW>
int launch_spread_batch(ovqe_handle h, bool stage, unsigned grid, size_t lds, const SparseArgs &A, const double *d_theta, const double *d_omega,
                        double w_energy, double w_spread, double *d_c, double *d_e, double *d_s, double *d_g) {
    constexpr auto staged = &k_sparse_spread_batch<NW, true>, plain = &k_sparse_spread_batch<NW, false>;
    if (int rc = lds_opt_in<staged, plain>(h, LDS_WG_MAX)) return rc;
    hipLaunchKernelGGL(stage ? staged : plain, dim3(grid), dim3(NW * 64), lds, h->stream, A, d_theta, (const SmallRot *)h->d_rots.p,
                       (const SpOp *)h->d_sp_ops.p, (const uint32_t *)h->d_sp_pairs.p, (const SpEntry *)h->d_sp_entries.p, d_omega, w_energy,
                       w_spread, d_c, d_e, d_s, d_g);
    HIPC(h, hipGetLastError());
    return OVQE_OK;
}

// *why != 0: path 1 does not serve the program (nothing was launched, info untouched).  omega: B values or null (omega_b = E_b);
// energies, spreads: may be null
int run_spread_batch(ovqe_handle h, int64_t B, const double *theta, const double *omega, double w_energy, double w_spread, double *costs,
                     double *grads, double *energies, double *spreads, int *why) {
    *why = spread::WHY_NO_COMPACT;
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
    // what ovqe_energy_gradient_batch takes its path 1 for
    if (!gradbatch::eligible(A) || !gradbatch::plan(A, B, h->opt_grad_batch_waves, h->opt_grad_batch_workgroups, handle_num_cus(h)).ok) return OVQE_OK;
    *why = spread::WHY_LDS;
    if (!spread::fits(A)) return OVQE_OK;
    const gradbatch::Plan G = spread::plan(A, B, h->opt_grad_batch_waves, h->opt_grad_batch_workgroups, handle_num_cus(h));
    if (!G.ok) return OVQE_OK;
    *why = spread::WHY_LEAK;
    if (h->sp_exact.leak) return OVQE_OK;
    *why = spread::WHY_ODD_Y;
    if (h->sp_exact.odd_y) return OVQE_OK;
    SpreadDev &D = spread_dev(h);
    if ((rc = ensure_events(h, D.ev, 3))) return rc;
    const size_t K = (size_t)h->K, rows = (size_t)B * K;
    if ((rc = ensure(h, D.d_theta, rows * sizeof(double)))) return rc;
    if (omega && (rc = ensure(h, D.d_omega, (size_t)B * sizeof(double)))) return rc;
    if ((rc = ensure(h, D.d_out, (3 * (size_t)B + rows) * sizeof(double)))) return rc;
    double *d_c = (double *)D.d_out.p, *d_e = d_c + B, *d_s = d_e + B, *d_g = d_s + B;
    const double *d_omega = omega ? (const double *)D.d_omega.p : nullptr;
    HIPC(h, hipEventRecord(D.ev[0], h->stream));
    HIPC(h, hipMemcpyAsync(D.d_theta.p, theta, rows * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (omega) HIPC(h, hipMemcpyAsync(D.d_omega.p, omega, (size_t)B * sizeof(double), hipMemcpyHostToDevice, h->stream));
    const unsigned grid = (unsigned)G.workgroups;
    const double *d_t = (const double *)D.d_theta.p;
    switch (G.nw) {
    case 1: rc = launch_spread_batch<1>(h, G.stage, grid, G.lds, A, d_t, d_omega, w_energy, w_spread, d_c, d_e, d_s, d_g); break;
    case 2: rc = launch_spread_batch<2>(h, G.stage, grid, G.lds, A, d_t, d_omega, w_energy, w_spread, d_c, d_e, d_s, d_g); break;
    case 4: rc = launch_spread_batch<4>(h, G.stage, grid, G.lds, A, d_t, d_omega, w_energy, w_spread, d_c, d_e, d_s, d_g); break;
    default: rc = launch_spread_batch<8>(h, G.stage, grid, G.lds, A, d_t, d_omega, w_energy, w_spread, d_c, d_e, d_s, d_g); break;
    }
    if (rc) return rc;
    HIPC(h, hipEventRecord(D.ev[1], h->stream));
    HIPC(h, hipMemcpyAsync(costs, d_c, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (energies) HIPC(h, hipMemcpyAsync(energies, d_e, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (spreads) HIPC(h, hipMemcpyAsync(spreads, d_s, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipMemcpyAsync(grads, d_g, rows * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipEventRecord(D.ev[2], h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    const int64_t info[11] = {1, B, (int64_t)K, omega ? 0 : 1, 1, G.stage ? 1 : 2, G.nw, G.workgroups, (int64_t)G.lds, h->sp_m, 0};
    std::copy(info, info + 11, D.info);
    if ((rc = phases_us(h, D.ev, 2, D.info + 11))) return rc;
    *why = spread::WHY_NONE;
    return OVQE_OK;
}
