// abi_gradbatch.inc — C-ABI entry points: exact gradients of a batch of parameter vectors (gradbatch_host.inc).
// Included by ovqe_sv.hip inside extern "C".

int ovqe_energy_gradient_batch(ovqe_handle h, int64_t B, const double *theta, int32_t K, double *energies, double *grads) try {
    OVQE_ENTER(h);
    if (!h) return OVQE_ERR_INVALID;
    if (B < 0) return fail(h, OVQE_ERR_INVALID, "ovqe_energy_gradient_batch: B is negative");
    // what ovqe_energy_gradient refuses, with its codes
    if (!h->prog_set) return fail(h, OVQE_ERR_STATE, "no program set (ovqe_set_program / ovqe_set_gate_program)");
    if (K != h->K) return fail(h, OVQE_ERR_INVALID, "K does not match the program's parameter count");
    if (!h->ham.set) return fail(h, OVQE_ERR_STATE, "no Hamiltonian set (ovqe_set_hamiltonian)");
    if (h->n_global) return fail(h, OVQE_ERR_INVALID, "ovqe_energy_gradient_batch is single-device, as ovqe_energy_gradient: not available on a shard handle");
    if (B == 0) return OVQE_OK;
    if (!energies) return fail(h, OVQE_ERR_INVALID, "ovqe_energy_gradient_batch: energies is NULL");
    if (K > 0 && (!theta || !grads)) return fail(h, OVQE_ERR_INVALID, std::string("ovqe_energy_gradient_batch: ") + (theta ? "grads" : "theta") + " is NULL");
    if (B > ((int64_t)1 << 40) / std::max<int64_t>(K, 1)) return fail(h, OVQE_ERR_INVALID, "ovqe_energy_gradient_batch: B x K is out of range");
    {
        FrameHamGuard frame_guard(h);   // an open Clifford frame: the rotations with the conjugated Hamiltonian, as the single call
        bool done = false;
        const int rc = run_grad_batch(h, B, theta, energies, grads, &done);
        if (rc || done) return rc;
    }
    // path 2: row by row through the single call (sector tables, streaming, literal gate lists); it takes its own frame guard
    double none = 0.0;   // (K = 0: the single call wants a gradient pointer and writes nothing through it)
    for (int64_t b = 0; b < B; ++b)
        if (int rc = energy_gradient_body(h, theta + b * K, K, energies + b, K > 0 ? grads + b * K : &none)) return rc;
    if (!h->grad_batch) h->grad_batch = new GradBatchDev();
    const int64_t info[11] = {2, B, K, 0, 0, 0, 0, 0, 0, 0, 0};
    std::copy(info, info + 11, h->grad_batch->info);
    return OVQE_OK;
} OVQE_CATCH(h)

int ovqe_gradient_batch_info(ovqe_handle h, int64_t *info, int count) try {
    OVQE_ENTER(h);
    if (!h || !info || count < 0) return OVQE_ERR_INVALID;
    for (int i = 0; i < count && i < 11; ++i) info[i] = h->grad_batch ? h->grad_batch->info[i] : 0;
    return OVQE_OK;
} OVQE_CATCH(h)
