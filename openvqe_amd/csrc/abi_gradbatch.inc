// abi_gradbatch.inc — C-ABI entry points: exact gradients of a batch of parameter vectors (gradbatch_host.inc).
// Included by ovqe_sv.hip inside extern "C".

int ovqe_energy_gradient_batch(ovqe_handle h, int64_t B, const double *theta, int32_t K, double *energies, double *grads) try {
    OVQE_ENTER(h);
    if (!h) return OVQE_ERR_INVALID;
    bool empty = false;
    const int refused = batch_refusals(h, {"ovqe_energy_gradient_batch", false, nullptr, "energies", energies}, B, theta, K, grads, &empty);
    if (refused || empty) return refused;
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
    return info_out(h, h && h->grad_batch ? h->grad_batch->info : nullptr, 11, info, count);
} OVQE_CATCH(h)
