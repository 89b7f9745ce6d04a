// constrain_host.inc — handle section of the observables beside the Hamiltonian: the Hermitian Pauli sums O_m a handle holds, and the
// compact path of ovqe_constrained_gradient_batch (kernel: k_sparse_constrained_batch in sv_sparse.hpp; the restriction rule:
// sv_constrain_host.hpp; entry points and the streaming path: abi_constrain.inc).  Included by ovqe_sv.hip inside its anonymous
// namespace.
//
// The observables belong to the register, as the deflation vectors do: nothing here looks at the program or the Hamiltonian, and setting
// either leaves them alone.  Each is kept as a grouped sum on the device (a HamDev: the streaming path applies it with
// apply_hamiltonian) and, for path 1, restricted to the compact support as SpEntry records — all observables one concatenated array.
// The entries are built lazily and cached: they are restricted again when the compact program was rebuilt (h->sp_build) or the set of
// observables changed (set_version) — the rule of the gathered deflation rows.  Path 1 is run_vqd_batch's (constrained_batch_plan restates its decision) with the
// deflation rows of deflate_host.inc.  Everything the calls allocate is this record's.

struct ConstrainDev {
    std::vector<HamDev *> obs;     // O_m: grouped terms on host and device, the constant
    int64_t set_version = 0;       // counts pushes and truncations
    // path 1
    std::vector<SpEntry> entries;  // all restricted observables, concatenated
    std::vector<int32_t> first;    // [M + 1]: observable m's entries are [first[m], first[m + 1])
    DevBuf d_entries, d_recs;
    int64_t entries_build = -1, entries_set = -1;
    DevBuf d_theta, d_out;         // rows [B * K]; costs [B], energies [B], gradients [B * K], row overlaps [B * rows], values [B * M]
    std::vector<double> h_d;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    int64_t info[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
};

void free_observable(HamDev *H) {
    if (!H) return;
    free_hamdev(*H);
    delete H;
}

void free_constrain(ConstrainDev *C) {
    if (!C) return;
    for (HamDev *H : C->obs) free_observable(H);
    for (DevBuf *b : {&C->d_entries, &C->d_recs, &C->d_theta, &C->d_out})
        if (b->p) (void)hipFree(b->p);
    for (hipEvent_t e : C->ev)
        if (e) (void)hipEventDestroy(e);
    delete C;
}

ConstrainDev &constrain_dev(ovqe_handle h) {
    if (!h->constrain) h->constrain = new ConstrainDev();
    return *h->constrain;
}

// the sum becomes observable M
int constrain_push(ovqe_handle h, int64_t T, const uint64_t *x, const uint64_t *z, const double *coeff, double constant) {
    ConstrainDev &C = constrain_dev(h);
    std::unique_ptr<HamDev, void (*)(HamDev *)> H(new HamDev(), free_observable);
    if (int rc = install_hamdev(h, *H, T, x, z, coeff, constant)) return rc;
    C.obs.push_back(H.get());
    (void)H.release();
    ++C.set_version;
    return OVQE_OK;
}

int constrain_truncate(ovqe_handle h, int32_t count) {
    ConstrainDev &C = constrain_dev(h);
    if ((size_t)count == C.obs.size()) return OVQE_OK;
    HIPC(h, hipStreamSynchronize(h->stream));
    while (C.obs.size() > (size_t)count) {
        free_observable(C.obs.back());
        C.obs.pop_back();
    }
    ++C.set_version;
    return OVQE_OK;
}

// the entries for the compact program and observable set of this moment; *builds: observables restricted (0: the cached entries serve)
int constrain_restrict(ovqe_handle h, ConstrainDev &C, int64_t *builds) {
    *builds = 0;
    if (C.entries_build == h->sp_build && C.entries_set == C.set_version) return OVQE_OK;
    const int slots = (int)h->sp_basis.size();
    std::unordered_map<uint64_t, int> slot_of;
    slot_of.reserve((size_t)slots);
    for (int k = 0; k < slots; ++k)
        if (h->sp_basis[(size_t)k] != ~0ull) slot_of.emplace(h->sp_basis[(size_t)k], k);
    C.entries.clear();
    C.first.assign(1, 0);
    for (const HamDev *H : C.obs) {
        std::vector<SpEntry> mine;
        if (!constrain::restrict_to_support(H->groups, H->terms, h->sp_basis.data(), slots, [&](uint64_t a) {
                auto it = slot_of.find(a);
                return it == slot_of.end() ? -1 : it->second;
            }, constrain::ENTRY_CAP, &mine) || C.entries.size() + mine.size() > constrain::ENTRY_CAP)
            return fail(h, OVQE_ERR_INVALID, "ovqe_constrained_gradient_batch: the observables restricted to the support exceed " +
                                                 std::to_string(constrain::ENTRY_CAP) + " entries");
        arrange_entries(mine);   // (the order of the Hamiltonian's stream: build_sparse_program)
        C.entries.insert(C.entries.end(), mine.begin(), mine.end());
        C.first.push_back((int32_t)C.entries.size());
        ++*builds;
    }
    if (int rc = upload(h, C.d_entries, C.entries.data(), C.entries.size() * sizeof(SpEntry))) return rc;
    C.entries_build = h->sp_build;
    C.entries_set = C.set_version;
    return OVQE_OK;
}

// Whether a batch of B rows runs on the compact support: run_vqd_batch's decision (deflate_host.inc), which is run_grad_batch's — same
// eligibility, same planner — with the kernel arguments and the launch geometry.  *ok = false: not eligible (nothing was launched).
int constrained_batch_plan(ovqe_handle h, int64_t B, SparseArgs *args, gradbatch::Plan *plan, bool *ok) {
    *ok = false;
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
    *args = A;
    *plan = G;
    *ok = true;
    return OVQE_OK;
}

template <int NW>
int launch_constrained_batch(ovqe_handle h, bool stage, unsigned grid, size_t lds, const SparseArgs &A, const double *d_theta, const DeflateDev &D,
                             const ConstrainDev &C, int M, double *d_c, double *d_e, double *d_g, double *d_d, double *d_v) {
    constexpr auto staged = &k_sparse_constrained_batch<NW, true>, plain = &k_sparse_constrained_batch<NW, false>;
    if (int rc = lds_opt_in<staged, plain>(h, LDS_WG_MAX)) return rc;
    hipLaunchKernelGGL(stage ? staged : plain, dim3(grid), dim3(NW * 64), lds, h->stream, A, d_theta, (const SmallRot *)h->d_rots.p,
                       (const SpOp *)h->d_sp_ops.p, (const uint32_t *)h->d_sp_pairs.p, (const SpEntry *)h->d_sp_entries.p,
                       (const double *)D.d_D.p, (const DeflRow *)D.d_rows.p, (int)D.rows.size(), (const SpEntry *)C.d_entries.p,
                       (const ConRec *)C.d_recs.p, M, d_c, d_e, d_g, d_d, d_v);
    HIPC(h, hipGetLastError());
    return OVQE_OK;
}

// *done = false: the program is not eligible for path 1 (nothing was launched, info untouched).  linear, quad, target: M doubles each
// (zeros where the caller gave none); energies, values, overlaps: may be null
int run_constrained_batch(ovqe_handle h, int64_t B, const double *theta, const double *linear, const double *quad, const double *target,
                          double *costs, double *grads, double *energies, double *values, double *overlaps, bool *done) {
    *done = false;
    int rc = OVQE_OK;
    SparseArgs A;
    gradbatch::Plan G;
    bool ok = false;
    if ((rc = constrained_batch_plan(h, B, &A, &G, &ok)) || !ok) return rc;
    DeflateDev &D = deflate_dev(h);
    ConstrainDev &C = constrain_dev(h);
    if ((rc = ensure_events(h, C.ev, 3))) return rc;
    int64_t gathers = 0, builds = 0;
    if ((rc = deflate_gather(h, D, A.mpad, &gathers))) return rc;
    if ((rc = constrain_restrict(h, C, &builds))) return rc;
    const size_t K = (size_t)h->K, rows = (size_t)B * K, J = D.vecs.size(), nr = D.rows.size(), M = C.obs.size();
    ConRec recs[constrain::OBS_MAX] = {};
    for (size_t m = 0; m < M; ++m)
        recs[m] = ConRec{C.first[m], C.first[m + 1] - C.first[m], C.obs[m]->constant, linear[m], quad[m], target[m]};
    if ((rc = ensure(h, C.d_recs, sizeof(recs)))) return rc;
    if ((rc = ensure(h, C.d_theta, rows * sizeof(double)))) return rc;
    if ((rc = ensure(h, C.d_out, (2 * (size_t)B + rows + (size_t)B * nr + (size_t)B * M) * sizeof(double)))) return rc;
    double *d_c = (double *)C.d_out.p, *d_e = d_c + B, *d_g = d_e + B, *d_d = d_g + rows, *d_v = d_d + (size_t)B * nr;
    HIPC(h, hipEventRecord(C.ev[0], h->stream));
    HIPC(h, hipMemcpyAsync(C.d_theta.p, theta, rows * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPC(h, hipMemcpyAsync(C.d_recs.p, recs, sizeof(recs), hipMemcpyHostToDevice, h->stream));
    const unsigned grid = (unsigned)G.workgroups;
    const double *d_theta = (const double *)C.d_theta.p;
    switch (G.nw) {
    case 1: rc = launch_constrained_batch<1>(h, G.stage, grid, G.lds, A, d_theta, D, C, (int)M, d_c, d_e, d_g, d_d, d_v); break;
    case 2: rc = launch_constrained_batch<2>(h, G.stage, grid, G.lds, A, d_theta, D, C, (int)M, d_c, d_e, d_g, d_d, d_v); break;
    case 4: rc = launch_constrained_batch<4>(h, G.stage, grid, G.lds, A, d_theta, D, C, (int)M, d_c, d_e, d_g, d_d, d_v); break;
    default: rc = launch_constrained_batch<8>(h, G.stage, grid, G.lds, A, d_theta, D, C, (int)M, d_c, d_e, d_g, d_d, d_v); break;
    }
    if (rc) return rc;
    HIPC(h, hipEventRecord(C.ev[1], h->stream));
    HIPC(h, hipMemcpyAsync(costs, d_c, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (energies) HIPC(h, hipMemcpyAsync(energies, d_e, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipMemcpyAsync(grads, d_g, rows * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (values && M) HIPC(h, hipMemcpyAsync(values, d_v, (size_t)B * M * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (overlaps && nr) {
        C.h_d.resize((size_t)B * nr);
        HIPC(h, hipMemcpyAsync(C.h_d.data(), d_d, (size_t)B * nr * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    }
    HIPC(h, hipEventRecord(C.ev[2], h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    if (overlaps && nr) deflate_overlaps_out(h, D, B, C.h_d.data(), overlaps);
    const int64_t info[14] = {1, B, (int64_t)K, (int64_t)M, (int64_t)J, (int64_t)nr, 1, G.stage ? 1 : 2, G.nw, G.workgroups, (int64_t)G.lds,
                              h->sp_m, (int64_t)C.entries.size(), builds};
    std::copy(info, info + 14, C.info);
    if ((rc = phases_us(h, C.ev, 2, C.info + 14))) return rc;
    *done = true;
    return OVQE_OK;
}
