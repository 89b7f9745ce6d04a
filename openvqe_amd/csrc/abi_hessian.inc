// abi_hessian.inc — C-ABI entry points: exact energy Hessian of the stored program (hessian_host.inc).
// Included by ovqe_sv.hip inside extern "C".

int ovqe_energy_hessian(ovqe_handle h, const double *theta, int32_t K, double *energy, double *grad, double *hess, double *asymmetry) try {
    OVQE_ENTER(h);
    if (!h) return OVQE_ERR_INVALID;
    if (!hess) return fail(h, OVQE_ERR_INVALID, "ovqe_energy_hessian: hess is NULL");
    if (h->n_global > 0) return fail(h, OVQE_ERR_STATE, "ovqe_energy_hessian: not available on a shard of a partitioned register");
    if (h->opt_real_state) return fail(h, OVQE_ERR_STATE, "ovqe_energy_hessian: not available under option real_state (the buffer holds 8-byte amplitudes)");
    if (!h->prog_set) return fail(h, OVQE_ERR_STATE, "ovqe_energy_hessian: no program set (ovqe_set_program / ovqe_set_gate_program)");
    if (!h->ham.set) return fail(h, OVQE_ERR_STATE, "ovqe_energy_hessian: no Hamiltonian set (ovqe_set_hamiltonian)");
    if (K != h->K) return fail(h, OVQE_ERR_INVALID, "ovqe_energy_hessian: K = " + std::to_string(K) + ", the program has " + std::to_string(h->K) + " parameters");
    if (K > 0 && !theta) return fail(h, OVQE_ERR_INVALID, "ovqe_energy_hessian: theta is NULL");
    if (asymmetry) *asymmetry = 0.0;
    if (K == 0) {   // no direction: the energy alone
        if (h->hessian) std::fill(h->hessian->info, h->hessian->info + 11, 0);
        double e = 0.0;
        const int rc = ovqe_energy(h, theta, 0, &e);
        if (!rc && energy) *energy = e;
        return rc;
    }
    FrameHamGuard frame_guard(h);   // an open Clifford frame: the rotations with the conjugated Hamiltonian, as every energy-type call
    return run_hessian(h, theta, energy, grad, hess, asymmetry);
} OVQE_CATCH(h)

int ovqe_hessian_info(ovqe_handle h, int64_t *info, int count) try {
    OVQE_ENTER(h);
    if (!h || !info || count < 0) return OVQE_ERR_INVALID;
    for (int i = 0; i < count && i < 11; ++i) info[i] = h->hessian ? h->hessian->info[i] : 0;
    return OVQE_OK;
} OVQE_CATCH(h)
