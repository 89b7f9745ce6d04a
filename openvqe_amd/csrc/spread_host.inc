// spread_host.inc — handle section of the energy spread S = ||(H - omega) psi||^2 with its gradient (geometry and eligibility:
// sv_spread_host.hpp; kernel: k_sparse_spread_batch in sv_sparse.hpp; entry points and the streaming path: abi_spread.inc).  Included
// by ovqe_sv.hip inside its anonymous namespace.
//
// Path 1 is run_grad_batch's — the handle's compact program as it stands, the whole batch in one launch — where three state arrays of
// one wave fit the budget AND the restricted entries are H on the support (h->sp_exact, decided once with the compact program in
// build_sparse_program).  Nothing is planned or built here beyond what the single gradient builds on its first use; everything the
// call allocates is this record's.

struct SpreadDev {
    BatchIo io;       // results: costs [B], energies [B], spreads [B], gradients [B * K]
    DevBuf d_omega;   // omega [B]
    int64_t info[13] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
};

void free_spread(SpreadDev *D) {
    if (!D) return;
    if (D->d_omega.p) (void)hipFree(D->d_omega.p);
    D->io.release();
    delete D;
}

SpreadDev &spread_dev(ovqe_handle h) {
    if (!h->spread) h->spread = new SpreadDev();
    return *h->spread;
}

// *why != 0: path 1 does not serve the program (nothing was launched, info untouched).  omega: B values or null (omega_b = E_b);
// energies, spreads: may be null
int run_spread_batch(ovqe_handle h, int64_t B, const double *theta, const double *omega, double w_energy, double w_spread, double *costs,
                     double *grads, double *energies, double *spreads, int *why) {
    *why = spread::WHY_NO_COMPACT;
    int rc = OVQE_OK;
    SparseArgs A;
    gradbatch::Plan G;
    bool ok = false;
    // what ovqe_energy_gradient_batch takes its path 1 for
    if ((rc = compact_batch_plan(h, B, &A, &G, &ok)) || !ok) return rc;
    *why = spread::WHY_LDS;
    if (!spread::fits(A)) return OVQE_OK;
    G = spread::plan(A, B, h->opt_grad_batch_waves, h->opt_grad_batch_workgroups, handle_num_cus(h));
    if (!G.ok) return OVQE_OK;
    *why = spread::WHY_LEAK;
    if (h->sp_exact.leak) return OVQE_OK;
    *why = spread::WHY_ODD_Y;
    if (h->sp_exact.odd_y) return OVQE_OK;
    SpreadDev &D = spread_dev(h);
    const size_t K = (size_t)h->K, rows = (size_t)B * K;
    if (omega && (rc = ensure(h, D.d_omega, (size_t)B * sizeof(double)))) return rc;
    if ((rc = D.io.begin(h, theta, rows, 3 * (size_t)B + rows))) return rc;
    double *d_c = (double *)D.io.d_out.p, *d_e = d_c + B, *d_s = d_e + B, *d_g = d_s + B;
    const double *d_omega = omega ? (const double *)D.d_omega.p : nullptr;
    if (omega) HIPC(h, hipMemcpyAsync(D.d_omega.p, omega, (size_t)B * sizeof(double), hipMemcpyHostToDevice, h->stream));
    rc = for_batch_waves(G.nw, [&](auto NW) {
        constexpr int nw = decltype(NW)::value;
        return launch_compact_batch<&k_sparse_spread_batch<nw, true>, &k_sparse_spread_batch<nw, false>>(h, G, A, D.io, d_omega, w_energy, w_spread,
                                                                                                        d_c, d_e, d_s, d_g);
    });
    if (rc) return rc;
    HIPC(h, hipMemcpyAsync(costs, d_c, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (energies) HIPC(h, hipMemcpyAsync(energies, d_e, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (spreads) HIPC(h, hipMemcpyAsync(spreads, d_s, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipMemcpyAsync(grads, d_g, rows * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if ((rc = D.io.end(h, D.info + 11))) return rc;
    const int64_t info[11] = {1, B, (int64_t)K, omega ? 0 : 1, 1, G.stage ? 1 : 2, G.nw, G.workgroups, (int64_t)G.lds, h->sp_m, 0};
    std::copy(info, info + 11, D.info);
    *why = spread::WHY_NONE;
    return OVQE_OK;
}

