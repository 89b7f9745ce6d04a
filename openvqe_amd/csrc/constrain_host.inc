// constrain_host.inc — handle section of the observables beside the Hamiltonian: the Hermitian Pauli sums O_m a handle holds, and the
// compact path of ovqe_constrained_gradient_batch (kernel: k_sparse_constrained_batch in sv_sparse.hpp; the restriction rule:
// sv_constrain_host.hpp; entry points and the streaming path: abi_constrain.inc).  Included by ovqe_sv.hip inside its anonymous
// namespace.
//
// The observables belong to the register, as the deflation vectors do: nothing here looks at the program or the Hamiltonian, and setting
// either leaves them alone.  Each is kept as a grouped sum on the device (a HamDev: the streaming path applies it with
// apply_hamiltonian) and, for path 1, restricted to the compact support as SpEntry records — all observables one concatenated array.
// The entries are built lazily and cached: they are restricted again when the compact program was rebuilt (h->sp_build) or the set of
// observables changed (set_version) — the rule of the gathered deflation rows.  Path 1 is run_vqd_batch's (compact_batch_plan) with
// the deflation rows of deflate_host.inc.  Everything the calls allocate is this record's.

struct ConstrainDev {
    std::vector<HamDev *> obs;     // O_m: grouped terms on host and device, the constant
    int64_t set_version = 0;       // counts pushes and truncations
    // path 1
    std::vector<SpEntry> entries;  // all restricted observables, concatenated
    std::vector<int32_t> first;    // [M + 1]: observable m's entries are [first[m], first[m + 1])
    DevBuf d_entries, d_recs;
    int64_t entries_build = -1, entries_set = -1;
    BatchIo io;                    // results: costs [B], energies [B], gradients [B * K], row overlaps [B * rows], values [B * M]
    std::vector<double> h_d;
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
    for (DevBuf *b : {&C->d_entries, &C->d_recs})
        if (b->p) (void)hipFree(b->p);
    C->io.release();
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

// *done = false: the program is not eligible for path 1 (nothing was launched, info untouched).  linear, quad, target: M doubles each
// (zeros where the caller gave none); energies, values, overlaps: may be null
int run_constrained_batch(ovqe_handle h, int64_t B, const double *theta, const double *linear, const double *quad, const double *target,
                          double *costs, double *grads, double *energies, double *values, double *overlaps, bool *done) {
    *done = false;
    int rc = OVQE_OK;
    SparseArgs A;
    gradbatch::Plan G;
    bool ok = false;
    if ((rc = compact_batch_plan(h, B, &A, &G, &ok)) || !ok) return rc;
    DeflateDev &D = deflate_dev(h);
    ConstrainDev &C = constrain_dev(h);
    int64_t gathers = 0, builds = 0;
    if ((rc = deflate_gather(h, D, A.mpad, &gathers))) return rc;
    if ((rc = constrain_restrict(h, C, &builds))) return rc;
    const size_t K = (size_t)h->K, rows = (size_t)B * K, J = D.vecs.size(), nr = D.rows.size(), M = C.obs.size();
    ConRec recs[constrain::OBS_MAX] = {};
    for (size_t m = 0; m < M; ++m)
        recs[m] = ConRec{C.first[m], C.first[m + 1] - C.first[m], C.obs[m]->constant, linear[m], quad[m], target[m]};
    if ((rc = ensure(h, C.d_recs, sizeof(recs)))) return rc;
    if ((rc = C.io.begin(h, theta, rows, 2 * (size_t)B + rows + (size_t)B * nr + (size_t)B * M))) return rc;
    double *d_c = (double *)C.io.d_out.p, *d_e = d_c + B, *d_g = d_e + B, *d_d = d_g + rows, *d_v = d_d + (size_t)B * nr;
    HIPC(h, hipMemcpyAsync(C.d_recs.p, recs, sizeof(recs), hipMemcpyHostToDevice, h->stream));
    rc = for_batch_waves(G.nw, [&](auto NW) {
        constexpr int nw = decltype(NW)::value;
        return launch_compact_batch<&k_sparse_constrained_batch<nw, true>, &k_sparse_constrained_batch<nw, false>>(
            h, G, A, C.io, (const double *)D.d_D.p, (const DeflRow *)D.d_rows.p, (int)D.rows.size(), (const SpEntry *)C.d_entries.p,
            (const ConRec *)C.d_recs.p, (int)M, d_c, d_e, d_g, d_d, d_v);
    });
    if (rc) return rc;
    HIPC(h, hipMemcpyAsync(costs, d_c, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (energies) HIPC(h, hipMemcpyAsync(energies, d_e, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipMemcpyAsync(grads, d_g, rows * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (values && M) HIPC(h, hipMemcpyAsync(values, d_v, (size_t)B * M * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (overlaps && nr) {
        C.h_d.resize((size_t)B * nr);
        HIPC(h, hipMemcpyAsync(C.h_d.data(), d_d, (size_t)B * nr * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    }
    if ((rc = C.io.end(h, C.info + 14))) return rc;
    if (overlaps && nr) deflate_overlaps_out(h, D, B, C.h_d.data(), overlaps);
    const int64_t info[14] = {1, B, (int64_t)K, (int64_t)M, (int64_t)J, (int64_t)nr, 1, G.stage ? 1 : 2, G.nw, G.workgroups, (int64_t)G.lds,
                              h->sp_m, (int64_t)C.entries.size(), builds};
    std::copy(info, info + 14, C.info);
    *done = true;
    return OVQE_OK;
}
