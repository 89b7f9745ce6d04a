// abi_spread.inc — C-ABI entry points: the energy spread S = ||(H - omega) psi||^2 (variance, folded-spectrum cost) with energies and
// exact gradients of a batch (spread_host.inc), and the streaming path.  Included by ovqe_sv.hip inside extern "C".

namespace {
// the two register-sized work vectors of a path-2 call: the call's own, freed when it leaves
struct SpreadWork {
    amp_t *sigma = nullptr, *tau = nullptr;
    ~SpreadWork() {
        if (sigma) (void)hipFree(sigma);
        if (tau) (void)hipFree(tau);
    }
    int alloc(ovqe_handle h) {
        const size_t bytes = (size_t)h->namps * sizeof(amp_t);
        for (amp_t **v : {&sigma, &tau})
            if (hipMalloc((void **)v, bytes) != hipSuccess) {
                (void)hipGetLastError();
                *v = nullptr;
                return fail(h, OVQE_ERR_ALLOC, "ovqe_spread_gradient_batch: hipMalloc of a work vector of " + std::to_string(bytes) + " bytes failed");
            }
        return OVQE_OK;
    }
};
constexpr int64_t SPREAD_ROW_LAUNCHES = 6;   // vector operations of a streaming row beyond the single gradient's: three axpy, one scale, k_dot and its k_reduce
}  // namespace

// One row on the streaming path, on the full complex register: psi = U(theta)|hf>, a = H psi without the constant (scratch[0]),
// E = Re <psi|a> + constant, sigma = a + s psi with s = constant - omega, S = <sigma|sigma>, tau = (H - omega) sigma (the Pauli-sum
// application with s as its identity part), lambda = w_energy a + w_spread tau in scratch[0], then the backward walk of
// ovqe_energy_gradient on (psi, lambda).  Dot products: k_dot's per-workgroup partials summed by k_reduce, the same bits from call to call.
static int spread_row_streaming(ovqe_handle h, const SpreadWork &W, const double *theta, int32_t K, const double *omega, double w_energy,
                                double w_spread, double *cost, double *grad, double *energy, double *spread) {
    const int rb = reduce_blocks(h->namps), nb = adjoint_walk_blocks(h);
    int rc = run_program_streaming(h, theta);
    if (!rc) rc = ensure_scratch(h, 0);
    if (!rc) rc = ensure(h, h->d_partials, (size_t)std::max(rb, ADJ_MAX_ROT * nb) * sizeof(double2));
    if (!rc) rc = ensure(h, h->d_result, 64 * sizeof(double2));
    if (rc) return rc;
    amp_t *lam = h->scratch[0];
    double2 e = make_double2(0.0, 0.0), s2 = make_double2(0.0, 0.0);
    rc = apply_hamiltonian(h, lam, h->state, 0.0);
    if (!rc) rc = vec_dot(h, h->state, lam, h->namps, &e);
    if (rc) return rc;
    const double E = e.x + h->ham.constant;
    const double s = h->ham.constant - (omega ? *omega : E);
    rc = vec_axpy(h, W.sigma, lam, 1.0, h->namps, true);
    if (!rc) rc = vec_axpy(h, W.sigma, h->state, s, h->namps, false);
    if (!rc) rc = vec_dot(h, W.sigma, W.sigma, h->namps, &s2);
    if (!rc) rc = apply_hamiltonian(h, W.tau, W.sigma, s);
    if (!rc) rc = vec_scale(h, lam, h->namps, w_energy);
    if (!rc) rc = vec_axpy(h, lam, W.tau, w_spread, h->namps, false);
    if (!rc) rc = adjoint_walk(h, lam, K, grad);
    if (rc) return rc;
    *energy = E;
    *spread = s2.x;
    *cost = w_energy * E + w_spread * s2.x;
    return OVQE_OK;
}

int ovqe_spread_gradient_batch(ovqe_handle h, int64_t B, const double *theta, int32_t K, const double *omega, double w_energy, double w_spread,
                               double *costs, double *grads, double *energies, double *spreads) try {
    OVQE_ENTER(h);
    if (!h) return OVQE_ERR_INVALID;
    bool empty = false;
    const int refused = batch_refusals(h, {"ovqe_spread_gradient_batch", true, nullptr, "costs", costs}, B, theta, K, grads, &empty, [&] {
        if (!std::isfinite(w_energy) || !std::isfinite(w_spread)) return fail(h, OVQE_ERR_INVALID, "ovqe_spread_gradient_batch: the weights must be finite");
        return (int)OVQE_OK;
    });
    if (refused || empty) return refused;
    if (omega)
        for (int64_t b = 0; b < B; ++b)
            if (!std::isfinite(omega[b])) return fail(h, OVQE_ERR_INVALID, "ovqe_spread_gradient_batch: omega[" + std::to_string(b) + "] is not finite");
    FrameHamGuard frame_guard(h);   // an open Clifford frame: the rotations with the conjugated Hamiltonian, which squares like any other
    int why = 0;
    {
        const int rc = run_spread_batch(h, B, theta, omega, w_energy, w_spread, costs, grads, energies, spreads, &why);
        if (rc || !why) return rc;
    }
    // path 2: row by row on the streaming kernels
    SpreadWork W;
    if (int rc = W.alloc(h)) return rc;
    double none = 0.0, e = 0.0, s = 0.0;   // (K = 0: nothing is written through the gradient pointer)
    for (int64_t b = 0; b < B; ++b) {
        if (int rc = spread_row_streaming(h, W, theta + b * K, K, omega ? omega + b : nullptr, w_energy, w_spread, costs + b,
                                          K > 0 ? grads + b * K : &none, &e, &s))
            return rc;
        if (energies) energies[b] = e;
        if (spreads) spreads[b] = s;
    }
    const int64_t info[13] = {2, B, K, omega ? 0 : 1, SPREAD_ROW_LAUNCHES * B, 0, 0, 0, 0, 0, why, 0, 0};
    std::copy(info, info + 13, spread_dev(h).info);
    return OVQE_OK;
} OVQE_CATCH(h)

int ovqe_spread_info(ovqe_handle h, int64_t *info, int count) try {
    OVQE_ENTER(h);
    return info_out(h, h && h->spread ? h->spread->info : nullptr, 13, info, count);
} OVQE_CATCH(h)
