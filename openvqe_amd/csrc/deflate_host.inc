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
    BatchIo io;                    // results: costs [B], energies [B], gradients [B * K], row overlaps [B * rows]
    std::vector<double> h_d;
    int64_t info[14] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
};

void free_deflate(DeflateDev *D) {
    if (!D) return;
    for (amp_t *v : D->vecs)
        if (v) (void)hipFree(v);
    for (DevBuf *b : {&D->d_D, &D->d_flags, &D->d_rows})
        if (b->p) (void)hipFree(b->p);
    D->io.release();
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
    int rc = OVQE_OK;
    SparseArgs A;
    gradbatch::Plan G;
    bool ok = false;
    if ((rc = compact_batch_plan(h, B, &A, &G, &ok)) || !ok) return rc;
    DeflateDev &D = deflate_dev(h);
    int64_t gathers = 0;
    if ((rc = deflate_gather(h, D, A.mpad, &gathers))) return rc;
    const size_t K = (size_t)h->K, rows = (size_t)B * K, J = D.vecs.size(), nr = D.rows.size();
    if ((rc = D.io.begin(h, theta, rows, 2 * (size_t)B + rows + (size_t)B * nr))) return rc;
    double *d_c = (double *)D.io.d_out.p, *d_e = d_c + B, *d_g = d_e + B, *d_d = d_g + rows;
    rc = for_batch_waves(G.nw, [&](auto NW) {
        constexpr int nw = decltype(NW)::value;
        return launch_compact_batch<&k_sparse_vqd_batch<nw, true>, &k_sparse_vqd_batch<nw, false>>(
            h, G, A, D.io, (const double *)D.d_D.p, (const DeflRow *)D.d_rows.p, (int)D.rows.size(), d_c, d_e, d_g, d_d);
    });
    if (rc) return rc;
    HIPC(h, hipMemcpyAsync(costs, d_c, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (energies) HIPC(h, hipMemcpyAsync(energies, d_e, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipMemcpyAsync(grads, d_g, rows * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (overlaps && nr) {
        D.h_d.resize((size_t)B * nr);
        HIPC(h, hipMemcpyAsync(D.h_d.data(), d_d, (size_t)B * nr * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    }
    if ((rc = D.io.end(h, D.info + 12))) return rc;
    if (overlaps && nr) deflate_overlaps_out(h, D, B, D.h_d.data(), overlaps);
    const int64_t info[12] = {1, B, (int64_t)K, (int64_t)J, (int64_t)nr, 1, G.stage ? 1 : 2, G.nw, G.workgroups, (int64_t)G.lds, h->sp_m, gathers};
    std::copy(info, info + 12, D.info);
    *done = true;
    return OVQE_OK;
}
