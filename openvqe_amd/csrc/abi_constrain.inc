// abi_constrain.inc — C-ABI entry points: the observables of a handle and costs of their expectation values with exact gradients
// (constrain_host.inc), and the streaming path of the latter.  Included by ovqe_sv.hip inside extern "C".

namespace {
// the register-sized work vector of a path-2 call: the call's own, freed when it leaves
struct ConstrainWork {
    amp_t *v = nullptr;
    ~ConstrainWork() {
        if (v) (void)hipFree(v);
    }
    int alloc(ovqe_handle h) {
        const size_t bytes = (size_t)h->namps * sizeof(amp_t);
        if (hipMalloc((void **)&v, bytes) != hipSuccess) {
            (void)hipGetLastError();
            v = nullptr;
            return fail(h, OVQE_ERR_ALLOC, "ovqe_constrained_gradient_batch: hipMalloc of the work vector of " + std::to_string(bytes) + " bytes failed");
        }
        return OVQE_OK;
    }
};
constexpr int64_t CONSTRAIN_OBS_LAUNCHES = 3;   // vector operations per observable of a streaming row: k_dot, its k_reduce, the axpy into lambda
}  // namespace

int ovqe_observable_push(ovqe_handle h, int64_t T, const uint64_t *x, const uint64_t *z, const double *coeff, double constant) try {
    OVQE_ENTER(h);
    if (!h || T < 0 || (T && (!x || !z || !coeff))) return OVQE_ERR_INVALID;
    if (h->n_global) return fail(h, OVQE_ERR_STATE, "ovqe_observable_push: not available on a shard of a partitioned register");
    if (h->opt_real_state) return fail(h, OVQE_ERR_STATE, "ovqe_observable_push: not available under option real_state (the buffer holds 8-byte amplitudes)");
    if (!std::isfinite(constant)) return fail(h, OVQE_ERR_INVALID, "ovqe_observable_push: the constant is not finite");
    for (int64_t t = 0; t < T; ++t)
        if (!std::isfinite(coeff[t])) return fail(h, OVQE_ERR_INVALID, "ovqe_observable_push: coeff[" + std::to_string(t) + "] is not finite");
    if (h->constrain && h->constrain->obs.size() >= (size_t)constrain::OBS_MAX)
        return fail(h, OVQE_ERR_INVALID, "ovqe_observable_push: a handle holds at most " + std::to_string(constrain::OBS_MAX) + " observables");
    return constrain_push(h, T, x, z, coeff, constant);
} OVQE_CATCH(h)

int ovqe_observable_truncate(ovqe_handle h, int32_t count) try {
    OVQE_ENTER(h);
    if (!h) return OVQE_ERR_INVALID;
    const size_t have = h->constrain ? h->constrain->obs.size() : 0;
    if (count < 0 || (size_t)count > have)
        return fail(h, OVQE_ERR_INVALID, "ovqe_observable_truncate: count is outside 0 .. " + std::to_string(have));
    if (!h->constrain) return OVQE_OK;
    return constrain_truncate(h, count);
} OVQE_CATCH(h)

int ovqe_observable_count(ovqe_handle h, int32_t *count) try {
    OVQE_ENTER(h);
    if (!h || !count) return OVQE_ERR_INVALID;
    *count = h->constrain ? (int32_t)h->constrain->obs.size() : 0;
    return OVQE_OK;
} OVQE_CATCH(h)

int ovqe_constrained_gradient_batch(ovqe_handle h, int64_t B, const double *theta, int32_t K, int32_t M, const double *linear, const double *quad,
                                    const double *target, double *costs, double *grads, double *energies, double *values,
                                    double *overlaps_re_im) try {
    OVQE_ENTER(h);
    if (!h) return OVQE_ERR_INVALID;
    double lin[constrain::OBS_MAX] = {}, qd[constrain::OBS_MAX] = {}, tg[constrain::OBS_MAX] = {};
    bool empty = false;
    const int refused = batch_refusals(
        h, {"ovqe_constrained_gradient_batch", true, "the observables and the stored vectors live", "costs", costs}, B, theta, K, grads, &empty, [&] {
            const int32_t held = h->constrain ? (int32_t)h->constrain->obs.size() : 0;
            if (M != held)
                return fail(h, OVQE_ERR_INVALID, "ovqe_constrained_gradient_batch: M = " + std::to_string(M) + ", the handle holds " + std::to_string(held) + " observables");
            for (int32_t m = 0; m < M; ++m) {
                if (linear) lin[m] = linear[m];
                if (quad) qd[m] = quad[m];
                if (target) tg[m] = target[m];
                if (!std::isfinite(lin[m]) || !std::isfinite(qd[m]) || !std::isfinite(tg[m]))
                    return fail(h, OVQE_ERR_INVALID, "ovqe_constrained_gradient_batch: a weight or the target of observable " + std::to_string(m) + " is not finite");
            }
            return (int)OVQE_OK;
        });
    if (refused || empty) return refused;
    {
        bool done = false;
        const int rc = run_constrained_batch(h, B, theta, lin, qd, tg, costs, grads, energies, values, overlaps_re_im, &done);
        if (rc || done) return rc;
    }
    // path 2: row by row on the streaming kernels — deflated_row_streaming with, per observable, work = O_m psi by the Pauli-sum
    // application, o_m = Re <psi|work> + constant_m, lambda += g_m work before the backward walk
    DeflateDev &D = deflate_dev(h);
    ConstrainDev &C = constrain_dev(h);
    const int64_t J = (int64_t)D.vecs.size();
    ConstrainWork W;
    if (M > 0)
        if (int rc = W.alloc(h)) return rc;
    double none = 0.0, e = 0.0, val[constrain::OBS_MAX] = {};   // (K = 0: nothing is written through the gradient pointer)
    double2 o[DEFLATE_MAX];
    int64_t launches = 0;
    for (int64_t b = 0; b < B; ++b) {
        const std::function<int(amp_t *, double *)> observables = [&](amp_t *lam, double *extra) {
            for (int32_t m = 0; m < M; ++m) {
                double2 d = make_double2(0.0, 0.0);
                int rc = apply_hamiltonian(h, W.v, h->state, 0.0, nullptr, 0, C.obs[(size_t)m]);
                if (!rc) rc = vec_dot(h, h->state, W.v, h->namps, &d);
                if (rc) return rc;
                const double om = d.x + C.obs[(size_t)m]->constant, dev = om - tg[m], g = lin[m] + 2.0 * qd[m] * dev;
                val[m] = om;
                *extra += lin[m] * om + qd[m] * dev * dev;
                if (g != 0.0 && (rc = vec_axpy(h, lam, W.v, g, h->namps, false))) return rc;
                launches += CONSTRAIN_OBS_LAUNCHES - (g != 0.0 ? 0 : 1);
            }
            return (int)OVQE_OK;
        };
        if (int rc = deflated_row_streaming(h, theta + b * K, K, costs + b, K > 0 ? grads + b * K : &none, &e, o, &launches, &observables)) return rc;
        if (energies) energies[b] = e;
        if (values) std::copy(val, val + M, values + b * M);
        if (overlaps_re_im) overlaps_out(overlaps_re_im, b, J, o);
    }
    const int64_t info[16] = {2, B, K, M, J, 0, launches, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    std::copy(info, info + 16, C.info);
    return OVQE_OK;
} OVQE_CATCH(h)

int ovqe_constraint_info(ovqe_handle h, int64_t *info, int count) try {
    OVQE_ENTER(h);
    return info_out(h, h && h->constrain ? h->constrain->info : nullptr, 16, info, count);
} OVQE_CATCH(h)
