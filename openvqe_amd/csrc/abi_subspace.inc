// abi_subspace.inc — C-ABI entry points: overlap and Hamiltonian matrices of a subspace expansion around the resident state
// (subspace_host.inc).  Included by ovqe_sv.hip inside extern "C".

int ovqe_subspace_matrices(ovqe_handle h, int64_t n_ops, const int64_t *offsets, const uint64_t *x, const uint64_t *z,
                           const double *coeff_re, const double *coeff_im, double *h_out_re_im, double *s_out_re_im) try {
    OVQE_ENTER(h);
    if (!h) return OVQE_ERR_INVALID;
    if (n_ops < 1) return fail(h, OVQE_ERR_INVALID, "ovqe_subspace_matrices: n_ops must be at least 1");
    if (!offsets) return fail(h, OVQE_ERR_INVALID, "ovqe_subspace_matrices: offsets is NULL");
    if (!s_out_re_im) return fail(h, OVQE_ERR_INVALID, "ovqe_subspace_matrices: s_out is NULL");
    if (h->n_global > 0) return fail(h, OVQE_ERR_STATE, "ovqe_subspace_matrices: not available on a shard of a partitioned register");
    if (h->opt_real_state)
        return fail(h, OVQE_ERR_STATE, "ovqe_subspace_matrices: not available under option real_state (the buffer holds 8-byte amplitudes)");
    if (h_out_re_im && !h->ham.set) return fail(h, OVQE_ERR_STATE, "ovqe_subspace_matrices: h_out asked for but no Hamiltonian set (ovqe_set_hamiltonian)");
    for (int64_t k = 0; k < n_ops; ++k)
        if (offsets[k] > offsets[k + 1] || offsets[k] < 0) return fail(h, OVQE_ERR_INVALID, "ovqe_subspace_matrices: offsets not monotone");
    const int64_t t0 = offsets[0], t1 = offsets[n_ops];
    if (t1 > t0 && (!x || !z || !coeff_re)) return fail(h, OVQE_ERR_INVALID, "ovqe_subspace_matrices: x, z or coeff_re is NULL");
    const uint64_t lmask = local_mask(h);
    for (int64_t t = t0; t < t1; ++t)
        if ((x[t] | z[t]) & ~lmask) return fail(h, OVQE_ERR_INVALID, "ovqe_subspace_matrices: Pauli mask has bits beyond the register");
    return run_subspace(h, n_ops, offsets, x, z, coeff_re, coeff_im, h_out_re_im, s_out_re_im);
} OVQE_CATCH(h)

int ovqe_subspace_info(ovqe_handle h, int64_t *info, int count) try {
    OVQE_ENTER(h);
    if (!h || !info || count < 0) return OVQE_ERR_INVALID;
    for (int i = 0; i < count && i < 20; ++i) info[i] = h->subspace ? h->subspace->info[i] : 0;
    return OVQE_OK;
} OVQE_CATCH(h)
