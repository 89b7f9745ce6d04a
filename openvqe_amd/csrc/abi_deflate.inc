// abi_deflate.inc — C-ABI entry points: the deflation vectors of a handle and deflated energies and gradients (deflate_host.inc), and
// the streaming path of the latter.  Included by ovqe_sv.hip inside extern "C".

// One row on the streaming path: psi = U(theta)|hf>, lambda = H psi, E = Re <psi|lambda>, o_j = <phi_j|psi> (k_deflate_dots, four vectors
// per pass, the blocks' partials summed by k_reduce into slot j of d_result), lambda += sum_j beta_j o_j phi_j (k_deflate_axpy, o_j read
// on the device), the backward walk of ovqe_energy_gradient on (psi, lambda).  *launches += the deflation launches made.
// more: null, or (*more)(lam, &extra) is what a caller adds to lambda before the walk and to the cost (abi_constrain.inc: the observables' terms).
static int deflated_row_streaming(ovqe_handle h, const double *theta, int32_t K, double *cost, double *grad, double *energy, double2 *o,
                                  int64_t *launches, const std::function<int(amp_t *, double *)> *more = nullptr) {
    DeflateDev &D = deflate_dev(h);
    const int J = (int)D.vecs.size(), rb = reduce_blocks(h->namps), nb = adjoint_walk_blocks(h);
    int rc = run_program_streaming(h, theta);
    if (!rc) rc = ensure_scratch(h, 0);
    if (!rc) rc = ensure(h, h->d_partials, (size_t)std::max(DEFLATE_CHUNK * rb, ADJ_MAX_ROT * nb) * sizeof(double2));
    if (!rc) rc = ensure(h, h->d_result, 64 * sizeof(double2));
    if (rc) return rc;
    amp_t *lam = h->scratch[0];
    double2 e = make_double2(0.0, 0.0);
    rc = apply_hamiltonian(h, lam, h->state, 0.0);
    if (!rc) rc = vec_dot(h, h->state, lam, h->namps, &e);
    if (rc) return rc;
    for (int j0 = 0; j0 < J; j0 += DEFLATE_CHUNK) {
        DeflChunk C = {};
        C.count = std::min(DEFLATE_CHUNK, J - j0);
        for (int k = 0; k < C.count; ++k) {
            C.v[k] = D.vecs[j0 + k];
            C.beta[k] = D.betas[j0 + k];
        }
        hipLaunchKernelGGL(k_deflate_dots, dim3(rb), dim3(256), 0, h->stream, C, (const amp_t *)h->state, h->namps, (double2 *)h->d_partials.p);
        HIPC(h, hipGetLastError());
        for (int k = 0; k < C.count; ++k)
            if ((rc = enqueue_reduce(h, (const double2 *)h->d_partials.p + (size_t)k * rb, rb, j0 + k))) return rc;
        hipLaunchKernelGGL(k_deflate_axpy, dim3(rb), dim3(256), 0, h->stream, C, (const double2 *)h->d_result.p + j0, lam, h->namps);
        HIPC(h, hipGetLastError());
        *launches += 2 + C.count;
    }
    if (J > 0 && (rc = fetch_result(h, o, J))) return rc;
    double extra = 0.0;
    if (more && (rc = (*more)(lam, &extra))) return rc;
    if ((rc = adjoint_walk(h, lam, K, grad))) return rc;
    double c = e.x + h->ham.constant;
    *energy = c;
    for (int j = 0; j < J; ++j) c += D.betas[j] * (o[j].x * o[j].x + o[j].y * o[j].y);
    *cost = c + extra;
    return OVQE_OK;
}

int ovqe_deflation_push(ovqe_handle h, double beta) try {
    OVQE_ENTER(h);
    if (!h) return OVQE_ERR_INVALID;
    if (h->n_global) return fail(h, OVQE_ERR_STATE, "ovqe_deflation_push: not available on a shard of a partitioned register");
    if (h->opt_real_state) return fail(h, OVQE_ERR_STATE, "ovqe_deflation_push: not available under option real_state (the buffer holds 8-byte amplitudes)");
    if (!std::isfinite(beta) || beta < 0.0) return fail(h, OVQE_ERR_INVALID, "ovqe_deflation_push: beta must be finite and not negative");
    if (h->deflate && h->deflate->vecs.size() >= (size_t)DEFLATE_MAX)
        return fail(h, OVQE_ERR_INVALID, "ovqe_deflation_push: a handle holds at most " + std::to_string(DEFLATE_MAX) + " vectors");
    return deflate_capture(h, beta);
} OVQE_CATCH(h)

int ovqe_deflation_truncate(ovqe_handle h, int32_t count) try {
    OVQE_ENTER(h);
    if (!h) return OVQE_ERR_INVALID;
    const size_t have = h->deflate ? h->deflate->vecs.size() : 0;
    if (count < 0 || (size_t)count > have)
        return fail(h, OVQE_ERR_INVALID, "ovqe_deflation_truncate: count is outside 0 .. " + std::to_string(have));
    if (!h->deflate) return OVQE_OK;
    return deflate_truncate(h, count);
} OVQE_CATCH(h)

int ovqe_deflation_count(ovqe_handle h, int32_t *count) try {
    OVQE_ENTER(h);
    if (!h || !count) return OVQE_ERR_INVALID;
    *count = h->deflate ? (int32_t)h->deflate->vecs.size() : 0;
    return OVQE_OK;
} OVQE_CATCH(h)

int ovqe_deflated_gradient_batch(ovqe_handle h, int64_t B, const double *theta, int32_t K, double *costs, double *grads, double *energies,
                                 double *overlaps_re_im) try {
    OVQE_ENTER(h);
    if (!h) return OVQE_ERR_INVALID;
    bool empty = false;
    const int refused = batch_refusals(h, {"ovqe_deflated_gradient_batch", true, "the stored vectors live", "costs", costs}, B, theta, K, grads, &empty);
    if (refused || empty) return refused;
    {
        bool done = false;
        const int rc = run_vqd_batch(h, B, theta, costs, grads, energies, overlaps_re_im, &done);
        if (rc || done) return rc;
    }
    // path 2: row by row on the streaming kernels
    DeflateDev &D = deflate_dev(h);
    const int64_t J = (int64_t)D.vecs.size();
    double none = 0.0, e = 0.0;   // (K = 0: nothing is written through the gradient pointer)
    double2 o[DEFLATE_MAX];
    int64_t launches = 0;
    for (int64_t b = 0; b < B; ++b) {
        if (int rc = deflated_row_streaming(h, theta + b * K, K, costs + b, K > 0 ? grads + b * K : &none, &e, o, &launches)) return rc;
        if (energies) energies[b] = e;
        if (overlaps_re_im) overlaps_out(overlaps_re_im, b, J, o);
    }
    const int64_t info[14] = {2, B, K, J, 0, launches, 0, 0, 0, 0, 0, 0, 0, 0};
    std::copy(info, info + 14, D.info);
    return OVQE_OK;
} OVQE_CATCH(h)

int ovqe_deflation_info(ovqe_handle h, int64_t *info, int count) try {
    OVQE_ENTER(h);
    return info_out(h, h && h->deflate ? h->deflate->info : nullptr, 14, info, count);
} OVQE_CATCH(h)
