// deflate_host.inc — handle section of variational quantum deflation: the vectors phi_j a handle holds with their weights beta_j, and the
// compact path of ovqe_deflated_gradient_batch (kernel: k_sparse_vqd_batch in sv_sparse.hpp; gather: sv_deflate.hpp; entry points and
// the streaming path: abi_deflate.inc).  Included by ovqe_sv.hip inside its anonymous namespace.
//
// The vectors belong to the register: nothing here looks at the program or the Hamiltonian, and setting either leaves them alone.
// Path 1 is run_grad_batch's — same eligibility, same planner, same LDS layout — with the vectors restricted to the compact support
// as real rows D (Re phi_j, and Im phi_j as a second row with the same weight where it is non-zero on the support; psi is zero off
// the support, so the restriction is exact).  D is cached: it is gathered again when the compact program was rebuilt (h->sp_build)
// or the set of vectors changed (set_version).  Everything the calls allocate is this record's.

struct DeflateDev {
    std::vector<amp_t *> vecs;     // phi_j: 2^n amplitudes each, device memory
    std::vector<double> betas;
    int64_t set_version = 0;       // counts pushes and truncations
    // path 1
    DevBuf d_D, d_flags, d_rows;   // rows [2 J][mpad] as gathered; Im-non-zero flags [J]; the rows in use (DeflRow)
    std::vector<DeflRow> rows;
    std::vector<int> row_vec;      // per row in use: its vector, and whether it is the imaginary part
    std::vector<uint8_t> row_im;
    int64_t gather_build = -1, gather_set = -1;
    DevBuf d_theta, d_out;         // rows [B * K]; costs [B], energies [B], gradients [B * K], row overlaps [B * rows]
    std::vector<double> h_d;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    int64_t info[14] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
};

void free_deflate(DeflateDev *D) {
    if (!D) return;
    for (amp_t *v : D->vecs)
        if (v) (void)hipFree(v);
    for (DevBuf *b : {&D->d_D, &D->d_flags, &D->d_rows, &D->d_theta, &D->d_out})
        if (b->p) (void)hipFree(b->p);
    for (hipEvent_t e : D->ev)
        if (e) (void)hipEventDestroy(e);
    delete D;
}

DeflateDev &deflate_dev(ovqe_handle h) {
    if (!h->deflate) h->deflate = new DeflateDev();
    return *h->deflate;
}

// a copy of the state buffer becomes vector J with weight beta
int deflate_capture(ovqe_handle h, double beta) {
    DeflateDev &D = deflate_dev(h);
    const size_t need = (size_t)h->namps * sizeof(amp_t);
    size_t free_b = 0, total_b = 0;
    HIPC(h, hipMemGetInfo(&free_b, &total_b));
    const size_t limit = free_b / 5 * 3;
    if (need > limit)
        return fail(h, OVQE_ERR_ALLOC, "ovqe_deflation_push: the vector needs " + std::to_string(need) + " bytes, the cap is " + std::to_string(limit) +
                                           " bytes (60 % of the free device memory)");
    amp_t *v = nullptr;
    if (hipMalloc((void **)&v, need) != hipSuccess) {
        (void)hipGetLastError();
        return fail(h, OVQE_ERR_ALLOC, "ovqe_deflation_push: hipMalloc of " + std::to_string(need) + " bytes failed");
    }
    if (hipMemcpyAsync(v, h->state, need, hipMemcpyDeviceToDevice, h->stream) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess) {
        (void)hipFree(v);
        return fail(h, OVQE_ERR_HIP, "ovqe_deflation_push: the copy of the state failed");
    }
    D.vecs.push_back(v);
    D.betas.push_back(beta);
    ++D.set_version;
    return OVQE_OK;
}

int deflate_truncate(ovqe_handle h, int32_t count) {
    DeflateDev &D = deflate_dev(h);
    if ((size_t)count == D.vecs.size()) return OVQE_OK;
    HIPC(h, hipStreamSynchronize(h->stream));
    while (D.vecs.size() > (size_t)count) {
        (void)hipFree(D.vecs.back());
        D.vecs.pop_back();
        D.betas.pop_back();
    }
    ++D.set_version;
    return OVQE_OK;
}

// D for the compact program and vector set of this moment; *launches: gather launches made (0: the cached rows serve)
int deflate_gather(ovqe_handle h, DeflateDev &D, int mpad, int64_t *launches) {
    *launches = 0;
    if (D.gather_build == h->sp_build && D.gather_set == D.set_version) return OVQE_OK;
    const int J = (int)D.vecs.size();
    D.rows.clear();
    D.row_vec.clear();
    D.row_im.clear();
    if (J > 0) {
        int rc = ensure(h, D.d_D, (size_t)2 * J * mpad * sizeof(double));
        if (!rc) rc = ensure(h, D.d_flags, (size_t)J * sizeof(int));
        if (rc) return rc;
        DeflVecs V = {};
        for (int j = 0; j < J; ++j) V.v[j] = D.vecs[j];
        HIPC(h, hipMemsetAsync(D.d_flags.p, 0, (size_t)J * sizeof(int), h->stream));
        hipLaunchKernelGGL(k_deflate_gather, dim3((unsigned)((mpad + 255) / 256), (unsigned)J), dim3(256), 0, h->stream, V,
                           (const uint64_t *)h->d_sp_basis.p, mpad, h->namps, (double *)D.d_D.p, (int *)D.d_flags.p);
        HIPC(h, hipGetLastError());
        *launches = 1;
        std::vector<int> flags((size_t)J, 0);
        HIPC(h, hipMemcpyAsync(flags.data(), D.d_flags.p, (size_t)J * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIPC(h, hipStreamSynchronize(h->stream));
        for (int j = 0; j < J; ++j)
            for (int im = 0; im < (flags[j] ? 2 : 1); ++im) {
                D.rows.push_back(DeflRow{D.betas[j], 2 * j + im, 0});
                D.row_vec.push_back(j);
                D.row_im.push_back((uint8_t)im);
            }
        if ((rc = upload(h, D.d_rows, D.rows.data(), D.rows.size() * sizeof(DeflRow)))) return rc;
    }
    D.gather_build = h->sp_build;
    D.gather_set = D.set_version;
    return OVQE_OK;
}

template <int NW>
int launch_vqd_batch(ovqe_handle h, bool stage, unsigned grid, size_t lds, const SparseArgs &A, const double *d_theta, const DeflateDev &D,
                     double *d_c, double *d_e, double *d_g, double *d_d) {
    constexpr auto staged = &k_sparse_vqd_batch<NW, true>, plain = &k_sparse_vqd_batch<NW, false>;
    if (int rc = lds_opt_in<staged, plain>(h, LDS_WG_MAX)) return rc;
    hipLaunchKernelGGL(stage ? staged : plain, dim3(grid), dim3(NW * 64), lds, h->stream, A, d_theta, (const SmallRot *)h->d_rots.p,
                       (const SpOp *)h->d_sp_ops.p, (const uint32_t *)h->d_sp_pairs.p, (const SpEntry *)h->d_sp_entries.p,
                       (const double *)D.d_D.p, (const DeflRow *)D.d_rows.p, (int)D.rows.size(), d_c, d_e, d_g, d_d);
    HIPC(h, hipGetLastError());
    return OVQE_OK;
}

// o_bj = <phi_j|psi> = init_amp (<Re phi_j|psi_c> - i <Im phi_j|psi_c>) from the row values d[B x rows in use] of a path-1 launch: the
// compact state starts from 1 at |hf>, the register from init_amp (the phase a folded Clifford part leaves)
void deflate_overlaps_out(ovqe_handle h, const DeflateDev &D, int64_t B, const double *d, double *overlaps) {
    const size_t J = D.vecs.size(), nr = D.rows.size();
    const double pr = h->init_amp.x, pi = h->init_amp.y;
    for (int64_t b = 0; b < B; ++b) {
        double *o = overlaps + (size_t)b * J * 2;
        std::fill(o, o + 2 * J, 0.0);
        for (size_t r = 0; r < nr; ++r) o[2 * D.row_vec[r] + D.row_im[r]] = D.row_im[r] ? -d[(size_t)b * nr + r] : d[(size_t)b * nr + r];
        if (pr != 1.0 || pi != 0.0)
            for (size_t j = 0; j < J; ++j) {
                const double re = o[2 * j], im = o[2 * j + 1];
                o[2 * j] = pr * re - pi * im;
                o[2 * j + 1] = pr * im + pi * re;
            }
    }
}

// *done = false: the program is not eligible for path 1 (nothing was launched, info untouched).  energies, overlaps: may be null
int run_vqd_batch(ovqe_handle h, int64_t B, const double *theta, double *costs, double *grads, double *energies, double *overlaps, bool *done) {
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
    DeflateDev &D = deflate_dev(h);
    if ((rc = ensure_events(h, D.ev, 3))) return rc;
    int64_t gathers = 0;
    if ((rc = deflate_gather(h, D, A.mpad, &gathers))) return rc;
    const size_t K = (size_t)h->K, rows = (size_t)B * K, J = D.vecs.size(), nr = D.rows.size();
    if ((rc = ensure(h, D.d_theta, rows * sizeof(double)))) return rc;
    if ((rc = ensure(h, D.d_out, (2 * (size_t)B + rows + (size_t)B * nr) * sizeof(double)))) return rc;
    double *d_c = (double *)D.d_out.p, *d_e = d_c + B, *d_g = d_e + B, *d_d = d_g + rows;
    HIPC(h, hipEventRecord(D.ev[0], h->stream));
    HIPC(h, hipMemcpyAsync(D.d_theta.p, theta, rows * sizeof(double), hipMemcpyHostToDevice, h->stream));
    const unsigned grid = (unsigned)G.workgroups;
    switch (G.nw) {
    case 1: rc = launch_vqd_batch<1>(h, G.stage, grid, G.lds, A, (const double *)D.d_theta.p, D, d_c, d_e, d_g, d_d); break;
    case 2: rc = launch_vqd_batch<2>(h, G.stage, grid, G.lds, A, (const double *)D.d_theta.p, D, d_c, d_e, d_g, d_d); break;
    case 4: rc = launch_vqd_batch<4>(h, G.stage, grid, G.lds, A, (const double *)D.d_theta.p, D, d_c, d_e, d_g, d_d); break;
    default: rc = launch_vqd_batch<8>(h, G.stage, grid, G.lds, A, (const double *)D.d_theta.p, D, d_c, d_e, d_g, d_d); break;
    }
    if (rc) return rc;
    HIPC(h, hipEventRecord(D.ev[1], h->stream));
    HIPC(h, hipMemcpyAsync(costs, d_c, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (energies) HIPC(h, hipMemcpyAsync(energies, d_e, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipMemcpyAsync(grads, d_g, rows * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (overlaps && nr) {
        D.h_d.resize((size_t)B * nr);
        HIPC(h, hipMemcpyAsync(D.h_d.data(), d_d, (size_t)B * nr * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    }
    HIPC(h, hipEventRecord(D.ev[2], h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    if (overlaps && nr) deflate_overlaps_out(h, D, B, D.h_d.data(), overlaps);
    const int64_t info[12] = {1, B, (int64_t)K, (int64_t)J, (int64_t)nr, 1, G.stage ? 1 : 2, G.nw, G.workgroups, (int64_t)G.lds, h->sp_m, gathers};
    std::copy(info, info + 12, D.info);
    if ((rc = phases_us(h, D.ev, 2, D.info + 12))) return rc;
    *done = true;
    return OVQE_OK;
}
