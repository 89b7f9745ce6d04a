// abi_adapt.inc — C-ABI entry points of the ADAPT screens (pool gradients, exact exponentials) and the non-zero list of the state.
// Included by ovqe_sv.hip inside extern "C".

// ---- ADAPT --------------------------------------------------------------------------------------
int ovqe_pool_gradients(ovqe_handle h, int64_t n_ops, const int64_t *offsets, const uint64_t *x, const uint64_t *z,
                        const double *coeff_re, const double *coeff_im, int mode, double *grads) try {
    OVQE_ENTER(h);
    if (!h || n_ops < 0 || !offsets || (n_ops && !grads)) return OVQE_ERR_INVALID;
    if (mode != OVQE_GRAD_FERMIONIC && mode != OVQE_GRAD_QUBIT) return fail(h, OVQE_ERR_INVALID, "unknown gradient mode");
    if (!h->ham.set) return fail(h, OVQE_ERR_STATE, "no Hamiltonian set (ovqe_set_hamiltonian)");
    if (n_ops == 0) return OVQE_OK;
    const int64_t T = offsets[n_ops];
    if (T < 0 || (T && (!x || !z || !coeff_re))) return OVQE_ERR_INVALID;
    for (int64_t k = 0; k < n_ops; ++k)
        if (offsets[k] > offsets[k + 1] || offsets[k] < 0) return fail(h, OVQE_ERR_INVALID, "offsets not monotone");
    int rc = ensure_scratch(h, 0);
    if (rc) return rc;
    amp_t *sig = h->scratch[0];
    const int nb = reduce_blocks(h->namps);
    // the support of psi, when it is a small part of the register (exact zeros outside: ovqe_apply_exp_pauli_sum and the
    // rotation sweeps never write an amplitude they do not reach)
    uint64_t support = 0;
    bool on_support = false;
    h->last_screen_support = -1;
    rc = list_support(h, &support, &on_support, 0);
    if (rc) return rc;
    if (on_support) h->last_screen_support = (int64_t)support;
    // sigma = H psi (constant included)
    bool sector_sigma = false;
    h->last_screen_sector = 0;
    if (on_support) {
        rc = screen_sector_sigma(h, sig, support, &sector_sigma);
        if (rc) return rc;
    }
    if (!sector_sigma) rc = apply_hamiltonian(h, sig, h->state, h->ham.constant, on_support ? (const uint64_t *)h->d_nz_idx.p : nullptr, support);
    if (rc) return rc;
    std::vector<double2> vals(n_ops);
    {
        // terms in caller order with i^ny folded.  The pool is the same host data on every ADAPT iteration: its device
        // copy lives on the handle and is uploaded again only when the content changes.
        const uint64_t lmask = local_mask(h);
        std::vector<HTerm> terms(T);
        std::vector<uint64_t> xs(T);
        for (int64_t t = 0; t < T; ++t) {
            if (x[t] & ~lmask) return fail(h, OVQE_ERR_INVALID, "x mask touches global (rank) bits");
            HTerm ht;
            ht.z = z[t];
            fold_iny(coeff_re[t], coeff_im ? coeff_im[t] : 0.0, __builtin_popcountll(x[t] & z[t]), ht.cr, ht.ci);
            terms[t] = ht;
            xs[t] = x[t];
        }
        const bool same = h->pg_valid && (int64_t)h->pg_off.size() == n_ops + 1 && (int64_t)h->pg_xs.size() == T &&
                          std::memcmp(h->pg_off.data(), offsets, (n_ops + 1) * sizeof(int64_t)) == 0 &&
                          (T == 0 || (std::memcmp(h->pg_xs.data(), xs.data(), T * sizeof(uint64_t)) == 0 &&
                                      std::memcmp(h->pg_terms.data(), terms.data(), T * sizeof(HTerm)) == 0));
        if (!same) {
            h->pg_valid = false;
            rc = upload(h, h->d_pg_off, offsets, (n_ops + 1) * sizeof(int64_t));
            if (!rc) rc = upload(h, h->d_pg_xs, xs.data(), std::max<int64_t>(T, 1) * sizeof(uint64_t));
            if (!rc) rc = upload(h, h->d_pg_terms, terms.data(), std::max<int64_t>(T, 1) * sizeof(HTerm));
            if (rc) return rc;
            h->pg_off.assign(offsets, offsets + n_ops + 1);
            h->pg_xs.swap(xs);
            h->pg_terms.swap(terms);
            h->pg_valid = true;
            // pattern tables of the same-x runs (see PoolRun)
            h->pg_tables = false;
            std::vector<PoolRun> runs((size_t)std::max<int64_t>(T, 1), PoolRun{0ull, 0u, -1, 0, 0});
            std::vector<double2> tabs;
            for (int64_t k = 0; k < n_ops; ++k)
                for (int64_t t = offsets[k]; t < offsets[k + 1];) {
                    int64_t te = t + 1;
                    while (te < offsets[k + 1] && h->pg_xs[te] == h->pg_xs[t]) ++te;
                    const uint64_t z0 = h->pg_terms[t].z;
                    uint64_t V = 0;
                    for (int64_t u = t; u < te; ++u) V |= h->pg_terms[u].z ^ z0;
                    const int nv = __builtin_popcountll(V);
                    if (te - t >= 2 && nv <= 4) {
                        PoolRun r{z0, 0u, nv, (int32_t)tabs.size(), 0};
                        int pos[4] = {0, 0, 0, 0}, c = 0;
                        for (uint64_t mk = V; mk; mk &= mk - 1ull) pos[c++] = __builtin_ctzll(mk);
                        r.vpos = (uint32_t)pos[0] | ((uint32_t)pos[1] << 6) | ((uint32_t)pos[2] << 12) | ((uint32_t)pos[3] << 18);
                        for (int pat = 0; pat < (1 << nv); ++pat) {
                            uint64_t bits = 0;   // the pattern placed on V
                            for (int b = 0; b < nv; ++b)
                                if ((pat >> b) & 1) bits |= 1ull << pos[b];
                            double dr = 0.0, di = 0.0;
                            for (int64_t u = t; u < te; ++u) {   // same terms, same order, fma: the device loop's doubles
                                const double sg = (__builtin_popcountll(bits & (h->pg_terms[u].z ^ z0)) & 1) ? -1.0 : 1.0;
                                dr = std::fma(h->pg_terms[u].cr, sg, dr);
                                di = std::fma(h->pg_terms[u].ci, sg, di);
                            }
                            tabs.push_back(make_double2(dr, di));
                        }
                        runs[t] = r;
                    }
                    t = te;
                }
            rc = upload(h, h->d_pg_runs, runs.data(), runs.size() * sizeof(PoolRun));
            if (tabs.empty()) tabs.push_back(make_double2(0.0, 0.0));
            if (!rc) rc = upload(h, h->d_pg_tabs, tabs.data(), tabs.size() * sizeof(double2));
            if (rc) return rc;
            h->pg_tables = true;
        }
        // one workgroup per operator while the state re-streams from L2/MALL; above that 2^16 amplitudes per workgroup
        const int nchunks = on_support ? (int)std::min<uint64_t>(256, (support + 65535) >> 16)
                                       : h->n_local <= 22 ? 1 : (int)(h->namps >> 16);
        const int64_t ops_per_launch = 32768;
        rc = ensure(h, h->d_pg_out, n_ops * sizeof(double2));
        if (!rc && nchunks > 1)
            rc = ensure(h, h->d_pg_part, (size_t)std::min<int64_t>(n_ops, ops_per_launch) * nchunks * sizeof(double2));
        if (rc) return rc;
        for (int64_t op0 = 0; op0 < n_ops; op0 += ops_per_launch) {
            const int64_t cnt = std::min<int64_t>(ops_per_launch, n_ops - op0);
            double2 *out = (double2 *)h->d_pg_out.p + op0;
            double2 *part = nchunks > 1 ? (double2 *)h->d_pg_part.p : out;
            if (on_support)
                hipLaunchKernelGGL(k_pool_grad_nz, dim3((unsigned)nchunks, (unsigned)cnt), dim3(256), 0, h->stream,
                                   (const amp_t *)sig, (const uint64_t *)h->d_nz_idx.p, (const amp_t *)h->d_nz_val.p, support,
                                   h->base, (const int64_t *)h->d_pg_off.p, (const uint64_t *)h->d_pg_xs.p,
                                   (const HTerm *)h->d_pg_terms.p, op0, part,
                                   h->pg_tables ? (const PoolRun *)h->d_pg_runs.p : (const PoolRun *)nullptr,
                                   (const double2 *)h->d_pg_tabs.p);
            else
                hipLaunchKernelGGL(k_pool_grad, dim3((unsigned)nchunks, (unsigned)cnt), dim3(256), 0, h->stream,
                                   (const amp_t *)sig, (const amp_t *)h->state, h->namps, h->base,
                                   (const int64_t *)h->d_pg_off.p, (const uint64_t *)h->d_pg_xs.p,
                                   (const HTerm *)h->d_pg_terms.p, op0, part);
            if (nchunks > 1)
                hipLaunchKernelGGL(k_reduce_rows2, dim3((unsigned)cnt), dim3(256), 0, h->stream, (const double2 *)part,
                                   nchunks, out);
        }
        hipError_t e = hipGetLastError();
        if (e == hipSuccess)
            e = hipMemcpyAsync(vals.data(), h->d_pg_out.p, n_ops * sizeof(double2), hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) return fail(h, OVQE_ERR_HIP, std::string("pool_gradients: ") + hipGetErrorString(e));
    }
    for (int64_t k = 0; k < n_ops; ++k)
        grads[k] = mode == OVQE_GRAD_FERMIONIC ? 2.0 * vals[k].x : 2.0 * std::hypot(vals[k].x, vals[k].y);
    return OVQE_OK;
} OVQE_CATCH(h)

int ovqe_apply_exp_pauli_sum(ovqe_handle h, int64_t T, const uint64_t *x, const uint64_t *z, const double *coeff_re,
                             const double *coeff_im, double theta) try {
    OVQE_ENTER(h);
    if (!h || T < 0 || (T && (!x || !z || !coeff_re))) return OVQE_ERR_INVALID;
    // the previous call on this handle left a list that contains the support (ovqe_init_basis, this function): see nz_super
    const bool have_list = h->nz_super_prev && h->own_state && !h->state_exposed && !h->opt_real_state;
    const uint64_t have_count = h->nz_super_count;
    if (T == 0 || theta == 0.0) {
        h->nz_super = have_list;   // nothing happens to the state
        return OVQE_OK;
    }
    std::vector<HGroup> groups;
    std::vector<HTerm> terms;
    int rc = build_groups(h, T, x, z, coeff_re, coeff_im, false, groups, terms);
    if (rc) return rc;
    double beta = 0.0;
    for (int64_t t = 0; t < T; ++t) beta += std::hypot(coeff_re[t], coeff_im ? coeff_im[t] : 0.0);
    beta *= std::fabs(theta);
    const int steps = std::max(1, (int)std::ceil(beta));
    const double tau = theta / steps, bstep = beta / steps;
    int M = 2;
    {
        double term = bstep * bstep / 2.0;
        while (term > 1e-19 && M < 64) {
            ++M;
            term *= bstep / M;
        }
    }
    rc = ensure_scratch(h, 0);
    if (!rc) rc = ensure_scratch(h, 1);
    if (rc) return rc;
    DevBuf &dg = h->d_exp_groups, &dt = h->d_exp_terms;   // (kept on the handle: an ADAPT run calls this hundreds of times)
    if (!rc) rc = upload(h, dg, groups.data(), groups.size() * sizeof(HGroup));
    if (!rc) rc = upload(h, dt, terms.data(), terms.size() * sizeof(HTerm));
    const int nb = reduce_blocks(h->namps);
    // A state of a few determinants (the ADAPT state while the ansatz is short): the series only reaches the closure of its
    // support under the operator's x-groups.  The closure is listed once ("screen_sparse" bounds it) and every Taylor step
    // runs over the list; amplitudes equal the pass over the register bit for bit.
    uint64_t reach = 0;
    bool listed = false;
    h->last_exp_support = -1;
    if (!rc && h->opt_screen_sparse > 0) {
        const uint64_t cap = h->namps / (uint64_t)h->opt_screen_sparse;
        if (have_list && have_count <= cap && h->d_nz_idx.p && h->d_nz_idx.cap >= cap * sizeof(uint64_t)) {
            reach = have_count;    // a superset of the support: its closure contains the support's, zeros cost nothing but their slots
            listed = true;
        } else {
            rc = list_support(h, &reach, &listed, cap);
        }
        if (!rc && listed) {
            const size_t words = (size_t)std::max<uint64_t>(1, h->namps >> 5);
            rc = ensure(h, h->d_nz_bitmap, words * sizeof(uint32_t) + 16);
            unsigned long long *d_total = nullptr;
            if (!rc) {
                d_total = (unsigned long long *)((char *)h->d_nz_bitmap.p + words * sizeof(uint32_t) + (8 - (words * sizeof(uint32_t)) % 8) % 8);
                unsigned long long t0 = reach;
                hipError_t e = hipMemsetAsync(h->d_nz_bitmap.p, 0, words * sizeof(uint32_t), h->stream);
                if (e == hipSuccess) e = hipMemcpyAsync(d_total, &t0, sizeof(t0), hipMemcpyHostToDevice, h->stream);
                if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
                if (e != hipSuccess) rc = fail(h, OVQE_ERR_HIP, "exp_pauli_sum: support bitmap");
            }
            if (!rc) {
                hipLaunchKernelGGL(k_support_mark, dim3((unsigned)((reach + 255) / 256)), dim3(256), 0, h->stream,
                                   (const uint64_t *)h->d_nz_idx.p, reach, (uint32_t *)h->d_nz_bitmap.p);
                uint64_t first = 0, last = reach;
                for (int round = 0; round < 4096 && !rc && listed && first < last; ++round) {
                    hipLaunchKernelGGL(k_support_expand, dim3((unsigned)((last - first + 255) / 256)), dim3(256), 0, h->stream,
                                       (uint64_t *)h->d_nz_idx.p, first, last, cap, h->base, (const HGroup *)dg.p, (int)groups.size(),
                                       (const HTerm *)dt.p, (uint32_t *)h->d_nz_bitmap.p, d_total);
                    unsigned long long total = 0;
                    hipError_t e = hipMemcpyAsync(&total, d_total, sizeof(total), hipMemcpyDeviceToHost, h->stream);
                    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
                    if (e != hipSuccess) rc = fail(h, OVQE_ERR_HIP, std::string("exp_pauli_sum: ") + hipGetErrorString(e));
                    if (total > cap) listed = false;   // the series fills too much of the register: walk it
                    first = last;
                    last = total;
                }
                reach = last;
            }
        }
    }
    if (!rc && listed) h->last_exp_support = (int64_t)reach;
    for (int s = 0; s < steps && !rc; ++s) {
        amp_t *va = h->scratch[0], *vb = h->scratch[1];
        // listed: the series lives on the list — the two work vectors are defined there only (k_apply_sum_list asks the bitmap)
        hipError_t e = hipSuccess;
        if (listed)
            hipLaunchKernelGGL(k_list_copy, dim3((unsigned)((reach + 255) / 256)), dim3(256), 0, h->stream, va, (const amp_t *)h->state,
                               (const uint64_t *)h->d_nz_idx.p, reach);
        else
            e = hipMemcpyAsync(va, h->state, h->namps * sizeof(amp_t), hipMemcpyDeviceToDevice, h->stream);
        if (e != hipSuccess) {
            rc = fail(h, OVQE_ERR_HIP, "exp_pauli_sum: copy failed");
            break;
        }
        for (int m = 1; m <= M; ++m) {
            if (listed)
                hipLaunchKernelGGL(k_apply_sum_list, dim3((unsigned)((reach + 255) / 256)), dim3(256), 0, h->stream, vb,
                                   (const amp_t *)va, h->state, (const uint64_t *)h->d_nz_idx.p, reach, h->base,
                                   (const HGroup *)dg.p, (int)groups.size(), (const HTerm *)dt.p, tau / m, 0.0,
                                   (const uint32_t *)h->d_nz_bitmap.p);
            else
                hipLaunchKernelGGL(k_apply_sum, dim3(nb), dim3(256), 0, h->stream, vb, (const amp_t *)va, h->state, h->namps,
                                   h->base, (const HGroup *)dg.p, (int)groups.size(), (const HTerm *)dt.p, tau / m, 0.0, 0.0,
                                   0.0);
            std::swap(va, vb);
        }
        if (hipGetLastError() != hipSuccess) rc = fail(h, OVQE_ERR_HIP, "exp_pauli_sum: launch failed");
    }
    if (!rc && hipStreamSynchronize(h->stream) != hipSuccess) rc = fail(h, OVQE_ERR_HIP, "exp_pauli_sum: sync failed");
    if (!rc && listed && h->own_state && !h->state_exposed) {
        h->nz_super = true;
        h->nz_super_count = reach;
    }
    return rc;
} OVQE_CATCH(h)

// ---- the state as a list of its non-zero amplitudes ---------------------------------------------------------------
int ovqe_get_support(ovqe_handle h, int64_t capacity, uint64_t *indices, double *amps, int64_t *count) try {
    OVQE_ENTER(h);
    if (!h || !count || capacity < 0 || (capacity && (!indices || !amps))) return OVQE_ERR_INVALID;
    *count = -1;
    if (h->n_global != 0 || h->namps < 4096) return OVQE_OK;   // small or sharded registers: ovqe_get_state
    const int keep = h->opt_screen_sparse;
    h->opt_screen_sparse = 1;   // list whatever the density
    uint64_t support = 0;
    bool listed = false;
    const int rc = list_support(h, &support, &listed, 0);
    h->opt_screen_sparse = keep;
    if (rc) return rc;
    *count = (int64_t)support;
    if (!listed || (int64_t)support > capacity) return OVQE_OK;   // (support = 0: nothing to copy)
    HIPC(h, hipMemcpyAsync(indices, h->d_nz_idx.p, support * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipMemcpyAsync(amps, h->d_nz_val.p, support * sizeof(amp_t), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    return OVQE_OK;
} OVQE_CATCH(h)
