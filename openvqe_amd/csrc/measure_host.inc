// measure_host.inc — handle section of finite-shot measurement (plan and geometry: sv_measure_host.hpp; kernels: sv_measure.hpp; entry
// points: abi_measure.inc).  Included by ovqe_sv.hip inside its anonymous namespace.
//
// One measurement = measure_state (basis change into scratch + prefix sums of |phi|^2) and measure_draw (shots, term signs, the fixed
// tree over the per-wave partials), all on the handle's stream.  The state buffer is only read.  ovqe_energy_sampled queues every
// group of the plan and waits once.

struct MeasureDev {
    DevBuf d_phi, d_cum, d_tot, d_idx, d_mask, d_coeff, d_tsum, d_part, d_vsum;
    DevBuf d_pmask, d_pcoeff;              // the plan's terms, group by group: x | z and coefficient
    measure::Plan plan;
    int plan_version = -1;                 // version of the stored Hamiltonian `plan` was built for
    std::vector<hipEvent_t> ev;            // four per measurement of the last call: start, basis change, scan, draw + score
    std::vector<double> host_vsum;
    int64_t info[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    int64_t launches = 0, high_passes = 0;
};

void free_measure(MeasureDev *M) {
    if (!M) return;
    for (DevBuf *b : {&M->d_phi, &M->d_cum, &M->d_tot, &M->d_idx, &M->d_mask, &M->d_coeff, &M->d_tsum, &M->d_part, &M->d_vsum, &M->d_pmask,
                      &M->d_pcoeff})
        if (b->p) (void)hipFree(b->p);
    for (hipEvent_t e : M->ev)
        if (e) (void)hipEventDestroy(e);
    delete M;
}

int measure_event(ovqe_handle h, MeasureDev &M, size_t k) {
    while (M.ev.size() <= k) {
        hipEvent_t e = nullptr;
        HIPC(h, hipEventCreate(&e));
        M.ev.push_back(e);
    }
    HIPC(h, hipEventRecord(M.ev[k], h->stream));
    return OVQE_OK;
}

MeasureDev &measure_dev(ovqe_handle h) {
    if (!h->measure) h->measure = new MeasureDev();
    return *h->measure;
}

// what every measuring entry point asks of its handle
int measure_applicable(ovqe_handle h, const char *who) {
    if (h->n_global > 0) return fail(h, OVQE_ERR_STATE, std::string(who) + ": not available on a shard of a partitioned register");
    if (h->opt_real_state) return fail(h, OVQE_ERR_STATE, std::string(who) + ": not available under option real_state (the buffer holds 8-byte amplitudes)");
    return OVQE_OK;
}

// the scratch of a measurement behind its cap: the prefix array, phi when a rotated bit lies above the tile
int measure_scratch(ovqe_handle h, MeasureDev &M, const measure::Geometry &G, const char *who) {
    const size_t want_phi = G.high.empty() ? 0 : G.phi_bytes;
    size_t need = 0;
    if (M.d_cum.cap < G.prefix_bytes) need += G.prefix_bytes;
    if (M.d_phi.cap < want_phi) need += want_phi;
    if (need) {
        size_t free_b = 0, total_b = 0;
        HIPC(h, hipMemGetInfo(&free_b, &total_b));
        const size_t limit = free_b / 5 * 3;
        if (need > limit)
            return fail(h, OVQE_ERR_ALLOC, std::string(who) + ": the measurement scratch needs " + std::to_string(need) + " bytes (" +
                                               std::to_string(G.prefix_bytes) + " for the prefix sums, " + std::to_string(want_phi) +
                                               " for the rotated state), the cap is " + std::to_string(limit) + " bytes (60 % of the free device memory)");
    }
    int rc = ensure(h, M.d_cum, G.prefix_bytes);
    if (!rc && want_phi) rc = ensure(h, M.d_phi, want_phi);
    if (!rc) rc = ensure(h, M.d_tot, G.totals_bytes);
    return rc;
}

// phi = B psi and the prefix sums of |phi|^2 into d_cum; events 4 m .. 4 m + 2
int measure_state(ovqe_handle h, MeasureDev &M, const measure::Geometry &G, size_t m) {
    const uint64_t N = h->namps;
    int rc = measure_event(h, M, 4 * m);
    if (rc) return rc;
    amp_t *phi = G.high.empty() ? nullptr : (amp_t *)M.d_phi.p;
    double *C = (double *)M.d_cum.p, *tot = (double *)M.d_tot.p;
    const size_t lds = (G.low_x | G.low_y) ? (sizeof(double2) << G.tile_bits) : 0;
    hipLaunchKernelGGL(k_meas_tile, dim3((unsigned)G.tiles), dim3(256), lds, h->stream, (const amp_t *)h->state, G.tile_bits, G.low_x, G.low_y, phi,
                       phi ? (double *)nullptr : C);
    HIPC(h, hipGetLastError());
    ++M.launches;
    for (size_t k = 0; k < G.high.size(); ++k) {   // the last pass above the tile writes p
        const uint64_t npairs = N >> 1;
        const unsigned gx = (unsigned)std::min<uint64_t>((npairs + 255) / 256, 1u << 20);
        hipLaunchKernelGGL(k_meas_high, dim3(gx), dim3(256), 0, h->stream, phi, npairs, G.high[k], G.high_y[k], k + 1 == G.high.size() ? C : (double *)nullptr);
        HIPC(h, hipGetLastError());
        ++M.launches;
        ++M.high_passes;
    }
    if ((rc = measure_event(h, M, 4 * m + 1))) return rc;
    hipLaunchKernelGGL(k_meas_scan_chunks, dim3((unsigned)G.chunks), dim3(measure::SCAN_THREADS), 0, h->stream, C, N, tot);
    HIPC(h, hipGetLastError());
    ++M.launches;
    if (G.chunks > 1) {
        hipLaunchKernelGGL(k_meas_scan_totals, dim3(1), dim3(256), 0, h->stream, tot, G.chunks);
        HIPC(h, hipGetLastError());
        hipLaunchKernelGGL(k_meas_scan_offsets, dim3((unsigned)(G.chunks - 1)), dim3(measure::SCAN_THREADS), 0, h->stream, C, N, (const double *)tot);
        HIPC(h, hipGetLastError());
        M.launches += 2;
    }
    return measure_event(h, M, 4 * m + 2);
}

// the shots of one measurement on the prefix sums in d_cum; slot `slot` of d_vsum takes (sum v, sum v^2, W); event 4 m + 3
int measure_draw(ovqe_handle h, MeasureDev &M, size_t m, int64_t n_shots, uint64_t seed, uint64_t stream, uint64_t first_shot, int T,
                 const uint64_t *d_mask, const double *d_coeff, unsigned long long *d_tsum, uint64_t *d_idx, int64_t slot) {
    const uint64_t key = mix64(seed ^ mix64(stream));
    const int64_t blocks = (n_shots + measure::DRAW_THREADS - 1) / measure::DRAW_THREADS, P = (n_shots + 63) / 64;
    int64_t L = 1;
    while (L < P) L <<= 1;
    const double *C = (const double *)M.d_cum.p;
    if (n_shots > 0) {
        hipLaunchKernelGGL(k_meas_draw, dim3((unsigned)blocks), dim3(measure::DRAW_THREADS), 0, h->stream, C, h->namps, n_shots, key, first_shot, T,
                           d_mask, d_coeff, d_tsum, (double2 *)M.d_part.p, d_idx);
        HIPC(h, hipGetLastError());
        ++M.launches;
    }
    hipLaunchKernelGGL(k_meas_finish, dim3(1), dim3(256), 0, h->stream, (double2 *)M.d_part.p, P, L, C, h->namps, (double *)M.d_vsum.p + 3 * slot);
    HIPC(h, hipGetLastError());
    ++M.launches;
    return measure_event(h, M, 4 * m + 3);
}

int measure_fill_info(ovqe_handle h, MeasureDev &M, int64_t groups, int64_t shots, int64_t terms) {
    M.info[0] = groups;
    M.info[1] = shots;
    M.info[2] = (int64_t)(M.d_cum.cap + M.d_phi.cap + M.d_tot.cap);
    M.info[3] = M.launches;
    double us[3] = {0.0, 0.0, 0.0};
    for (int64_t m = 0; m < groups; ++m)
        for (int k = 0; k < 3; ++k) {
            float ms = 0.f;
            HIPC(h, hipEventElapsedTime(&ms, M.ev[4 * m + k], M.ev[4 * m + k + 1]));
            us[k] += 1e3 * ms;
        }
    for (int k = 0; k < 3; ++k) M.info[4 + k] = (int64_t)us[k];
    M.info[7] = terms;
    M.info[8] = M.high_passes;
    return OVQE_OK;
}

int measure_check_norm(ovqe_handle h, double W, const char *who) {
    if (W > 0.0 && std::isfinite(W)) return OVQE_OK;
    return fail(h, OVQE_ERR_STATE, std::string(who) + ": the state has no weight to draw from (sum of |amplitude|^2 = " + std::to_string(W) + ")");
}

// ovqe_sample / ovqe_measure_paulis
int run_measure(ovqe_handle h, uint64_t xbasis, uint64_t ybasis, int64_t n_shots, uint64_t seed, uint64_t stream, uint64_t first_shot, int64_t T,
                const uint64_t *mask, const double *coeff, int64_t *term_sums, double *value_sums, uint64_t *indices, const char *who) {
    MeasureDev &M = measure_dev(h);
    std::fill(M.info, M.info + 9, 0);
    M.launches = M.high_passes = 0;
    const measure::Geometry G = measure::geometry(h->n_local, xbasis, ybasis);
    int rc = measure_scratch(h, M, G, who);
    const int64_t blocks = (n_shots + measure::DRAW_THREADS - 1) / measure::DRAW_THREADS;
    if (!rc) rc = ensure(h, M.d_part, (size_t)std::max<int64_t>(blocks * 4, 1) * sizeof(double2));
    if (!rc) rc = ensure(h, M.d_vsum, 3 * sizeof(double));
    if (!rc && T) rc = upload(h, M.d_mask, mask, (size_t)T * sizeof(uint64_t));
    if (!rc && T) rc = upload(h, M.d_coeff, coeff, (size_t)T * sizeof(double));
    if (!rc && T) rc = ensure(h, M.d_tsum, (size_t)T * sizeof(int64_t));
    if (!rc && indices && n_shots) rc = ensure(h, M.d_idx, (size_t)n_shots * sizeof(uint64_t));
    if (rc) return rc;
    if (T) HIPC(h, hipMemsetAsync(M.d_tsum.p, 0, (size_t)T * sizeof(int64_t), h->stream));
    if ((rc = measure_state(h, M, G, 0))) return rc;
    if ((rc = measure_draw(h, M, 0, n_shots, seed, stream, first_shot, (int)T, (const uint64_t *)M.d_mask.p, (const double *)M.d_coeff.p,
                           T ? (unsigned long long *)M.d_tsum.p : nullptr, indices && n_shots ? (uint64_t *)M.d_idx.p : nullptr, 0)))
        return rc;
    double vs[3] = {0.0, 0.0, 0.0};
    HIPC(h, hipMemcpyAsync(vs, M.d_vsum.p, sizeof(vs), hipMemcpyDeviceToHost, h->stream));
    if (T) HIPC(h, hipMemcpyAsync(term_sums, M.d_tsum.p, (size_t)T * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    if (indices && n_shots) HIPC(h, hipMemcpyAsync(indices, M.d_idx.p, (size_t)n_shots * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    if ((rc = measure_fill_info(h, M, 1, n_shots, T))) return rc;
    if ((rc = measure_check_norm(h, vs[2], who))) return rc;
    if (value_sums) {
        value_sums[0] = vs[0];
        value_sums[1] = vs[1];
    }
    return OVQE_OK;
}

// the measurement plan of the stored Hamiltonian (as the caller gave it), rebuilt when the Hamiltonian changed
int measure_plan(ovqe_handle h, MeasureDev &M) {
    if (M.plan_version == h->ham.version) return OVQE_OK;
    M.plan_version = -1;
    const int64_t T = (int64_t)h->user_x.size();
    M.plan = measure::plan_groups(T, h->user_x.data(), h->user_z.data(), h->user_c.data());
    M.plan.constant += h->user_const;
    std::vector<uint64_t> pm;
    std::vector<double> pc;
    for (int32_t t : M.plan.members) {
        pm.push_back(h->user_x[t] | h->user_z[t]);
        pc.push_back(h->user_c[t]);
    }
    int rc = upload(h, M.d_pmask, pm.data(), pm.size() * sizeof(uint64_t));   // (upload waits: the vectors may go)
    if (!rc) rc = upload(h, M.d_pcoeff, pc.data(), pc.size() * sizeof(double));
    if (rc) return rc;
    M.plan_version = h->ham.version;
    return OVQE_OK;
}

// ovqe_energy_sampled, behind the state preparation: every group with stream = its number, shots 0 .. n_shots - 1; one wait
int run_energy_sampled(ovqe_handle h, int64_t n_shots, uint64_t seed, double *energy, double *std_error) {
    const char *who = "ovqe_energy_sampled";
    MeasureDev &M = measure_dev(h);
    std::fill(M.info, M.info + 9, 0);
    M.launches = M.high_passes = 0;
    int rc = measure_plan(h, M);
    if (rc) return rc;
    const measure::Plan &P = M.plan;
    const int64_t G = P.groups();
    const int64_t blocks = (n_shots + measure::DRAW_THREADS - 1) / measure::DRAW_THREADS;
    if ((rc = ensure(h, M.d_part, (size_t)std::max<int64_t>(blocks * 4, 1) * sizeof(double2)))) return rc;
    if ((rc = ensure(h, M.d_vsum, (size_t)std::max<int64_t>(G, 1) * 3 * sizeof(double)))) return rc;
    for (int64_t g = 0; g < G; ++g) {
        const measure::Geometry Gm = measure::geometry(h->n_local, P.xbasis[g], P.ybasis[g]);
        if ((rc = measure_scratch(h, M, Gm, who))) return rc;
        if ((rc = measure_state(h, M, Gm, (size_t)g))) return rc;
        const int64_t f = P.first[g], Tg = P.first[g + 1] - f;
        if ((rc = measure_draw(h, M, (size_t)g, n_shots, seed, (uint64_t)g, 0, (int)Tg, (const uint64_t *)M.d_pmask.p + f, (const double *)M.d_pcoeff.p + f,
                               nullptr, nullptr, g)))
            return rc;
    }
    M.host_vsum.assign((size_t)G * 3, 0.0);
    if (G) HIPC(h, hipMemcpyAsync(M.host_vsum.data(), M.d_vsum.p, (size_t)G * 3 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    if ((rc = measure_fill_info(h, M, G, n_shots, (int64_t)P.members.size()))) return rc;
    std::vector<double> sv((size_t)G), sv2((size_t)G);
    for (int64_t g = 0; g < G; ++g) {
        if ((rc = measure_check_norm(h, M.host_vsum[3 * g + 2], who))) return rc;
        sv[g] = M.host_vsum[3 * g];
        sv2[g] = M.host_vsum[3 * g + 1];
    }
    measure::estimate(P.constant, n_shots, sv, sv2, energy, std_error);
    return OVQE_OK;
}
