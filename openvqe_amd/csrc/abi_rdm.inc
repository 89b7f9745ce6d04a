// abi_rdm.inc — C-ABI entry points: one- and two-particle density matrices of the resident state (rdm_host.inc).
// Included by ovqe_sv.hip inside extern "C".

int ovqe_rdm(ovqe_handle h, int order, double *out_re_im) try {
    OVQE_ENTER(h);
    if (!h) return OVQE_ERR_INVALID;
    if (!out_re_im) return fail(h, OVQE_ERR_INVALID, "ovqe_rdm: out is NULL");
    if (order != 1 && order != 2) return fail(h, OVQE_ERR_INVALID, "ovqe_rdm: order must be 1 or 2");
    if (h->n_global > 0) return fail(h, OVQE_ERR_STATE, "ovqe_rdm: not available on a shard of a partitioned register");
    if (h->opt_real_state) return fail(h, OVQE_ERR_STATE, "ovqe_rdm: not available under option real_state (the buffer holds 8-byte amplitudes)");
    if (order == 2 && h->n_local < 2) return fail(h, OVQE_ERR_INVALID, "ovqe_rdm: order 2 needs at least two orbitals");
    return run_rdm(h, order, out_re_im);
} OVQE_CATCH(h)

int ovqe_rdm_info(ovqe_handle h, int64_t *info, int count) try {
    OVQE_ENTER(h);
    if (!h || !info || count < 0) return OVQE_ERR_INVALID;
    for (int i = 0; i < count && i < 12; ++i) info[i] = h->rdm ? h->rdm->info[i] : 0;
    return OVQE_OK;
} OVQE_CATCH(h)
