// abi_solvers.inc — C-ABI entry points: device Lanczos (whole register and sector tables) and the adjoint gradient.
// Included by ovqe_sv.hip inside extern "C".

// ---- vector operations of the Lanczos recurrence ----------------------------------------------------------------------------------
// One launcher each, for RegisterSpace below, the ovqe_vec_* entry points and the <H> of ovqe_energy_gradient.  Operands are device
// buffers read as `nel` double2 elements; the reductions need d_partials for reduce_blocks(nel) sums and d_result (vec_reduce_prepare).
namespace {

inline uint64_t vec_elements(ovqe_handle h) { return h->opt_real_state ? std::max<uint64_t>(h->namps >> 1, 1) : h->namps; }
int vec_reduce_prepare(ovqe_handle h, int nb) {
    int rc = ensure(h, h->d_partials, (size_t)nb * sizeof(double2));
    if (!rc) rc = ensure(h, h->d_result, 64 * sizeof(double2));
    return rc;
}
int vec_dot(ovqe_handle h, const amp_t *a, const amp_t *b, uint64_t nel, double2 *out) {
    const int nb = reduce_blocks(nel);
    hipLaunchKernelGGL(k_dot, dim3(nb), dim3(256), 0, h->stream, a, b, nel, (double2 *)h->d_partials.p);
    return reduce_to_host(h, h->d_partials.p, nb, out);
}
// w -= alpha v + beta vprev (vprev may be null);  *norm2 = |w|^2
int vec_update(ovqe_handle h, amp_t *w, const amp_t *v, const amp_t *vprev, double alpha, double beta, uint64_t nel, double *norm2) {
    const int nb = reduce_blocks(nel);
    hipLaunchKernelGGL(k_lanczos_update, dim3(nb), dim3(256), 0, h->stream, w, v, vprev, alpha, beta, nel, (double2 *)h->d_partials.p);
    return reduce_to_host(h, h->d_partials.p, nb, norm2);
}
int vec_scale(ovqe_handle h, amp_t *v, uint64_t nel, double s) {
    hipLaunchKernelGGL(k_scale, dim3(reduce_blocks(nel)), dim3(256), 0, h->stream, v, nel, s);
    HIPC(h, hipGetLastError());
    return OVQE_OK;
}
int vec_axpy(ovqe_handle h, amp_t *y, const amp_t *x, double s, uint64_t nel, bool overwrite) {
    hipLaunchKernelGGL(k_axpy_real, dim3(reduce_blocks(nel)), dim3(256), 0, h->stream, y, x, s, nel, overwrite ? 1 : 0);
    HIPC(h, hipGetLastError());
    return OVQE_OK;
}
// the seeded fill of a whole register (complex amplitudes), normalised
int vec_start(ovqe_handle h, amp_t *v, uint64_t seed) {
    const int nb = reduce_blocks(h->namps);
    hipLaunchKernelGGL(k_randomize, dim3(nb), dim3(256), 0, h->stream, v, h->namps, h->base, seed, 1.0, (double2 *)h->d_partials.p);
    double n2 = 0.0;
    if (int rc = reduce_to_host(h, h->d_partials.p, nb, &n2)) return rc;
    return vec_scale(h, v, h->namps, 1.0 / std::sqrt(n2));
}

// ---- ground state of the stored Hamiltonian: Lanczos on the device -------------------------------------------
// The whole register as a Lanczos space (sv_lanczos_host.hpp): work vectors scratch[0], scratch[1] and `tmp`, the Ritz vector in h->state.
// One pass while the Lanczos vectors fit in HBM (24 qubits: 256 MiB each, 150 of them = 40 GB of the 288): v_0..v_j stay
// where they were written and the Ritz vector is their combination.  Beyond the budget ("lanczos_keep_gb", and never more
// than 60 % of the free memory) the kept vectors are dropped and the recurrence is run a second time for the Ritz vector.
struct RegisterSpace {
    typedef amp_t *Vec;
    ovqe_handle h;
    amp_t *tmp;
    uint64_t seed;
    const size_t vec_bytes = h->namps * sizeof(amp_t);
    size_t keep_budget = 0;
    bool keeping = false;
    std::vector<amp_t *> kept;
    RegisterSpace(ovqe_handle h, amp_t *tmp, uint64_t seed) : h(h), tmp(tmp), seed(seed) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess)
            keep_budget = std::min<size_t>((size_t)std::max(h->opt_lanczos_keep_gb, 0) << 30, free_b / 5 * 3);
        keeping = keep_budget >= 8 * vec_bytes;
    }
    Vec work(int i) const { return i == 2 ? tmp : h->scratch[i]; }
    Vec ritz() const { return h->state; }
    int start(Vec v) { return vec_start(h, v, seed); }
    int apply(Vec out, Vec in) { return apply_hamiltonian(h, out, in, 0.0); }
    int dot(Vec a, Vec b, double *re) {
        double2 d = make_double2(0.0, 0.0);
        const int rc = vec_dot(h, a, b, h->namps, &d);
        *re = d.x;
        return rc;
    }
    int update(Vec w, Vec v, Vec vprev, double alpha, double beta, double *norm2) {
        return vec_update(h, w, v, vprev, alpha, beta, h->namps, norm2);
    }
    int scale(Vec v, double a) { return vec_scale(h, v, h->namps, a); }
    int axpy(Vec y, Vec x, double a, bool first) { return vec_axpy(h, y, x, a, h->namps, first); }
    void drop_kept() {
        for (amp_t *v : kept) (void)hipFree(v);
        kept.clear();
        keeping = false;
    }
    int keep(Vec vj) {
        if (!keeping) return OVQE_OK;
        // v_j has served as v_{j-1}'s successor: a copy stays in `kept` from here on, as long as the budget lasts — a device-to-device
        // copy at HBM rate (0.1 ms at 24 qubits) next to a 40 ms H psi.  The first vector that cannot be kept drops them all.
        amp_t *fresh = nullptr;
        if ((kept.size() + 1) * vec_bytes <= keep_budget && hipMalloc((void **)&fresh, vec_bytes) == hipSuccess &&
            hipMemcpyAsync(fresh, vj, vec_bytes, hipMemcpyDeviceToDevice, h->stream) == hipSuccess) {
            kept.push_back(fresh);
            return OVQE_OK;
        }
        (void)hipGetLastError();
        if (fresh) (void)hipFree(fresh);
        drop_kept();
        return OVQE_OK;
    }
    int ritz_from_kept(const std::vector<double> &s, int m, bool *done) {
        *done = keeping && (int)kept.size() == m - 1;
        if (!*done) return OVQE_OK;   // (then nothing is held: keep() drops all or none)
        // kept = v_0..v_{m-2}; v_{m-1} is the vector the last step multiplied, still in its work buffer: scratch[(m-1) % 3 ...]
        // (the rotation A <- B <- C <- A moves one buffer per step, starting from B = scratch[1])
        amp_t *ring[3] = {h->scratch[1], tmp, h->scratch[0]};
        for (int j = 0; j < m; ++j)
            if (int rc = axpy(h->state, j < m - 1 ? kept[j] : ring[(m - 1) % 3], s[j], j == 0)) return rc;
        return OVQE_OK;
    }
    int release_kept() {
        const bool synced = hipStreamSynchronize(h->stream) == hipSuccess;
        drop_kept();
        return synced ? OVQE_OK : fail(h, OVQE_ERR_HIP, "ground_state: sync failed");
    }
};

}  // namespace

extern "C" int ovqe_ground_state(ovqe_handle h, double tol, int max_iter, uint64_t seed, double *energy,
                                 double *residual, int *iterations) try {
    OVQE_ENTER(h);
    if (!h || !energy || max_iter < 1 || !(tol > 0.0)) return OVQE_ERR_INVALID;
    if (!h->ham.set) return fail(h, OVQE_ERR_STATE, "no Hamiltonian set (ovqe_set_hamiltonian)");
    if (h->n_global) return fail(h, OVQE_ERR_INVALID, "ovqe_ground_state is single-device");
    int rc = ensure_scratch(h, 0);
    if (!rc) rc = ensure_scratch(h, 1);
    if (!rc) rc = vec_reduce_prepare(h, reduce_blocks(h->namps));
    if (rc) return rc;
    max_iter = (int)std::min<uint64_t>((uint64_t)max_iter, h->namps);
    amp_t *tmp = nullptr;
    if (hipMalloc((void **)&tmp, h->namps * sizeof(amp_t)) != hipSuccess) return fail(h, OVQE_ERR_ALLOC, "hipMalloc Lanczos vector");
    RegisterSpace V(h, tmp, seed);
    LanczosResult res;
    rc = lanczos_lowest(V, tol, max_iter, res);
    if (!rc && hipGetLastError() != hipSuccess) rc = fail(h, OVQE_ERR_HIP, "ground_state: launch failed");
    (void)hipFree(tmp);
    if (rc) return rc;
    *energy = res.lam + h->ham.constant;
    if (residual) *residual = res.residual;
    if (iterations) *iterations = res.m;
    return OVQE_OK;
} OVQE_CATCH(h)

// ---- Lanczos vector operations on caller-held shard buffers ----------------------------------------------------------------------
// What RegisterSpace does inside ovqe_ground_state, for a host layer that runs the recurrence over a partitioned register
// (openvqe_amd/distributed.py: ShardedStatevector.ground_state).  Operands are device buffers of the handle's storage: 2^n_local
// amp_t, or 2^n_local doubles under "real_state" — the kernels read a buffer as double2 elements, and a real buffer is half as many
// elements with the same sums.  Every value returned is the partial of THIS shard: the caller reduces over the ranks.
extern "C" int ovqe_vec_dot(ovqe_handle h, const void *a_dev, const void *b_dev, double *out_re_im) try {
    OVQE_ENTER(h);
    if (!h || !a_dev || !b_dev || !out_re_im) return OVQE_ERR_INVALID;
    const uint64_t nel = vec_elements(h);
    if (int rc = vec_reduce_prepare(h, reduce_blocks(nel))) return rc;
    double2 r;
    if (int rc = vec_dot(h, (const amp_t *)a_dev, (const amp_t *)b_dev, nel, &r)) return rc;
    out_re_im[0] = r.x;
    out_re_im[1] = h->opt_real_state ? 0.0 : r.y;   // (the y sum of doubles read as pairs means nothing)
    return OVQE_OK;
} OVQE_CATCH(h)

extern "C" int ovqe_vec_lanczos_update(ovqe_handle h, void *w_dev, const void *v_dev, const void *vprev_dev, double alpha, double beta,
                                       double *norm2_out) try {
    OVQE_ENTER(h);
    if (!h || !w_dev || !v_dev || !norm2_out) return OVQE_ERR_INVALID;
    if (w_dev == v_dev || w_dev == vprev_dev) return fail(h, OVQE_ERR_INVALID, "ovqe_vec_lanczos_update: w must differ from v and v_prev");
    const uint64_t nel = vec_elements(h);
    if (int rc = vec_reduce_prepare(h, reduce_blocks(nel))) return rc;
    return vec_update(h, (amp_t *)w_dev, (const amp_t *)v_dev, (const amp_t *)vprev_dev, alpha, beta, nel, norm2_out);
} OVQE_CATCH(h)

extern "C" int ovqe_vec_scale(ovqe_handle h, void *v_dev, double s) try {
    OVQE_ENTER(h);
    if (!h || !v_dev) return OVQE_ERR_INVALID;
    return vec_scale(h, (amp_t *)v_dev, vec_elements(h), s);
} OVQE_CATCH(h)

extern "C" int ovqe_vec_axpy(ovqe_handle h, void *y_dev, const void *x_dev, double s, int overwrite) try {
    OVQE_ENTER(h);
    if (!h || !y_dev || !x_dev) return OVQE_ERR_INVALID;
    return vec_axpy(h, (amp_t *)y_dev, (const amp_t *)x_dev, s, vec_elements(h), overwrite != 0);
} OVQE_CATCH(h)

// ---- lowest eigenpair inside the support of the stored program (sector tables) ------------------------------------
extern "C" int ovqe_sector_ground_state(ovqe_handle h, double tol, int max_iter, uint64_t seed, double *energy, double *residual,
                                        int *iterations) try {
    OVQE_ENTER(h);
    if (!h || !energy || max_iter < 1 || !(tol > 0.0)) return OVQE_ERR_INVALID;
    if (!h->ham.set) return fail(h, OVQE_ERR_STATE, "no Hamiltonian set (ovqe_set_hamiltonian)");
    if (!h->prog_set) {
        // no program: the sector of the state in the buffer — the closure of its support under the Hamiltonian's x-groups, e.g. of
        // the Hartree-Fock determinant after ovqe_init_basis: the (N_alpha, N_beta) sector, no UCCSD program needed to name it
        if (!h->opt_sector || h->n_global != 0) return fail(h, OVQE_ERR_STATE, "no program set, and the sector of the current state needs option sector on one device");
        uint64_t support = 0;
        bool listed = false;
        int rc = list_support(h, &support, &listed, 0);
        if (rc) return rc;
        if (!listed) return fail(h, OVQE_ERR_STATE, "no program set, and the state in the buffer is empty or not sparse (ovqe_init_basis first)");
        SectorEngine &S = h->scr;
        if (S.valid && S.ham_version != h->ham.version) free_sector(S);
        if (S.valid) {   // does the state live in the sector these tables were built for ?
            HIPC(h, hipMemsetAsync(S.d_buf[0].p, 0, (size_t)S.K * sizeof(double), h->stream));
            HIPC(h, hipMemsetAsync(S.d_flag.p, 0, sizeof(int), h->stream));
            hipLaunchKernelGGL(k_scr_compact, dim3((unsigned)((support + 255) / 256)), dim3(256), 0, h->stream, (const uint64_t *)h->d_nz_idx.p,
                               (const double2 *)h->d_nz_val.p, support, (const uint32_t *)S.d_sup.p, S.K, (double *)S.d_buf[0].p, (int *)S.d_flag.p);
            int flag = 0;
            HIPC(h, hipMemcpyAsync(&flag, S.d_flag.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
            HIPC(h, hipStreamSynchronize(h->stream));
            if (flag & 1) free_sector(S);
        }
        if (!S.valid) {
            rc = build_screen_sector(h, support);
            if (rc) return rc;
        }
        if (!S.valid) return fail(h, OVQE_ERR_STATE, "no sector tables for the current state (complex Hamiltonian, closure denser than 1/sector_sparsity, or tables beyond sector_max_gb)");
        // the Lanczos block starts from the first listed determinant of the state
        uint64_t first_index = 0;
        HIPC(h, hipMemcpyAsync(&first_index, h->d_nz_idx.p, sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
        HIPC(h, hipStreamSynchronize(h->stream));
        std::vector<uint32_t> sup(S.K);
        HIPC(h, hipMemcpyAsync(sup.data(), S.d_sup.p, (size_t)S.K * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
        HIPC(h, hipStreamSynchronize(h->stream));
        const auto it = std::lower_bound(sup.begin(), sup.end(), (uint32_t)first_index);
        if (it == sup.end() || *it != (uint32_t)first_index) return fail(h, OVQE_ERR_STATE, "internal: state outside its own sector");
        S.hf_final = (uint32_t)(it - sup.begin());
        return run_sector_ground_state(h, S, tol, max_iter, seed, energy, residual, iterations);
    }
    FrameHamGuard frame_guard(h);
    const bool real = h->opt_real_stream && h->prog_real_ok && h->n_global == 0 && tile_ok(h, true) && h->ham.groups.size() >= 3;
    if (!real || !h->opt_sector) return fail(h, OVQE_ERR_STATE, "the stored program has no sector tables (real-amplitude program on one device needed)");
    SectorEngine &E = h->sec;
    if (E.prog_version != h->prog_version || E.ham_version != h->ham.version) {
        free_sector(E);
        E.disabled = false;
        E.seen = 0;
        E.probe_mode = 0;
        E.coset_rejected = false;
        E.prog_version = h->prog_version;
        E.ham_version = h->ham.version;
    }
    if (!E.valid && !E.disabled) {   // built on demand here: this call is what the tables are for
        int rc = build_sector(h);
        if (rc) return rc;
    }
    if (!E.valid || !E.h_tables)
        return fail(h, OVQE_ERR_STATE, "the stored program has no sector tables (support too dense, or the tables exceed sector_max_gb)");
    int rc = run_sector_ground_state(h, h->sec, tol, max_iter, seed, energy, residual, iterations);
    // Lanczos diagonalised C^+ H C on the rotation-only program's support: the vector in the buffer is C^+ |psi0>; the header
    // promises the eigenvector of the caller's H there (fidelities are taken against it), so the Clifford part goes on top
    if (!rc && h->frame_open) rc = apply_tail_gates(h);
    return rc;
} OVQE_CATCH(h)

// ---- exact gradient by the adjoint method -------------------------------------------------------------------
// The backward walk of the streaming path, for ovqe_energy_gradient and ovqe_deflated_gradient_batch: psi = U(theta)|hf> in h->state,
// lambda (H psi, or H psi plus what the caller added) in `lam`; the op list is walked backwards on both and grad[0..K) takes
// 2 Re <lambda| dU/dtheta_k ...>.  adjoint_walk_blocks: the workgroups of its sweeps — one pair per thread while that stays below
// 65536 workgroups (a grid-stride loop of dependent load -> rotate -> store trips exposes the memory latency of both states), partial
// sums per workgroup and rotation in d_partials (the caller sizes it: ADJ_MAX_ROT x blocks doubles at the least).
static int adjoint_walk_blocks(ovqe_handle h) { return (int)std::min<uint64_t>(65536, std::max<uint64_t>(1, (h->namps / 2 + 255) / 256)); }
static int adjoint_walk(ovqe_handle h, amp_t *lam, int32_t K, double *grad) {
    const int nb = adjoint_walk_blocks(h);
    const size_t R = h->rots.size(), S = h->srots.size();
    DevBuf d_w;
    int rc = ensure(h, d_w, std::max<size_t>(R, 1) * sizeof(double));
    if (rc) return rc;
    const RotParam *d_rp = (const RotParam *)h->d_rp.p + S;
    double *partials = (double *)h->d_partials.p;
    for (int oi = (int)h->ops.size() - 1; oi >= 0 && !rc; --oi) {
        const SmallOp &op = h->ops[oi];
        switch (op.kind) {
        case OP_PAIR:
        case OP_DIAG:
            for (int hi = op.count; hi > 0; hi -= ADJ_MAX_ROT) {  // chunks from the end of the run backwards
                const int lo = std::max(0, hi - ADJ_MAX_ROT), cnt = hi - lo;
                if (op.kind == OP_PAIR)
                    hipLaunchKernelGGL(k_adjoint_pairs, dim3(nb), dim3(256), 0, h->stream, h->state, lam, h->namps >> 1,
                                       op.pivot, op.x, h->base, d_rp + op.first + lo, cnt, partials);
                else
                    hipLaunchKernelGGL(k_adjoint_diag, dim3(nb), dim3(256), 0, h->stream, h->state, lam, h->namps,
                                       h->base, d_rp + op.first + lo, cnt, partials);
                hipLaunchKernelGGL(k_reduce_rows, dim3(cnt), dim3(256), 0, h->stream, (const double *)partials, nb,
                                   (double *)d_w.p + op.first + lo);
            }
            break;
        case OP_X:
            rc = launch_gate(h, 0, op.pivot, 0);
            if (!rc) rc = launch_gate(h, 0, op.pivot, 0, lam);
            break;
        case OP_H:
            rc = launch_gate(h, 1, op.pivot, 0);
            if (!rc) rc = launch_gate(h, 1, op.pivot, 0, lam);
            break;
        case OP_CNOT:
            rc = launch_gate(h, 2, op.first, op.count);
            if (!rc) rc = launch_gate(h, 2, op.first, op.count, lam);
            break;
        default: rc = fail(h, OVQE_ERR_INVALID, "corrupt program");
        }
    }
    std::vector<double> w(R, 0.0);
    if (!rc && hipGetLastError() != hipSuccess) rc = fail(h, OVQE_ERR_HIP, "energy_gradient: launch failed");
    if (!rc && R && hipMemcpyAsync(w.data(), d_w.p, R * sizeof(double), hipMemcpyDeviceToHost, h->stream) != hipSuccess)
        rc = fail(h, OVQE_ERR_HIP, "energy_gradient: copy failed");
    if (!rc && hipStreamSynchronize(h->stream) != hipSuccess) rc = fail(h, OVQE_ERR_HIP, "energy_gradient: sync failed");
    if (d_w.p) (void)hipFree(d_w.p);
    if (rc) return rc;
    for (int32_t p = 0; p < K; ++p) grad[p] = 0.0;
    for (size_t r = 0; r < R; ++r) {
        const SmallRot &sr = h->rots[r];
        if (sr.pidx >= 0) grad[sr.pidx] += 2.0 * sr.coeff * ((sr.ny & 2) ? -w[r] : w[r]);
    }
    return OVQE_OK;
}

// (the body of ovqe_energy_gradient; ovqe_energy_gradient_batch serves the rows of a program without a batched form through it)
static int energy_gradient_body(ovqe_handle h, const double *theta, int32_t K, double *energy, double *grad) {
    int rc = check_theta(h, theta, K);
    if (rc) return rc;
    if (!h->ham.set) return fail(h, OVQE_ERR_STATE, "no Hamiltonian set (ovqe_set_hamiltonian)");
    if (h->n_global) return fail(h, OVQE_ERR_INVALID, "ovqe_energy_gradient is single-device: on a shard handle run the backward steps with ovqe_adjoint_rotations "
                                                     "(openvqe_amd/distributed.py: program_energy_gradient)");
    FrameHamGuard frame_guard(h);
    {   // small registers: forward, H psi and the backward pass in one launch on the compact support
        bool done = false;
        rc = run_sparse_gradient(h, theta, energy, grad, &done);
        if (rc || done) return rc;
    }
    if (h->opt_real_stream && h->prog_real_ok && tile_ok(h, true) && h->ham.groups.size() >= 3) {
        // real-amplitude program on a sparse support: the whole adjoint pass on the sector tables
        rc = sector_prepare(h, true);
        if (rc) return rc;
        if (h->sec.valid && h->sec.h_tables && sector_gradient_fits(h)) {   // (else: tiles sized for energies only, "sector_tile_cap")
            bool ok = false;
            rc = run_sector_gradient(h, theta, energy, grad, &ok);
            if (rc || ok) return rc;
            sector_orphaned(h);
            if (!h->sec.disabled) {   // second attempt: support probed with independent angles
                rc = sector_prepare(h, true);
                if (rc) return rc;
                if (h->sec.valid && h->sec.h_tables && sector_gradient_fits(h)) {
                    rc = run_sector_gradient(h, theta, energy, grad, &ok);
                    if (rc || ok) return rc;
                    sector_orphaned(h);
                }
            }
        }
    }
    rc = run_program_streaming(h, theta);  // psi = U(theta)|hf>; angle table: original rotations at offset S
    if (!rc) rc = ensure_scratch(h, 0);
    // the backward sweeps' partial sums per workgroup and rotation (adjoint_walk)
    const int nb = adjoint_walk_blocks(h);
    if (!rc) rc = ensure(h, h->d_partials, (size_t)std::max(reduce_blocks(h->namps), ADJ_MAX_ROT * nb) * sizeof(double2));
    if (!rc) rc = ensure(h, h->d_result, 64 * sizeof(double2));
    if (rc) return rc;
    amp_t *lam = h->scratch[0];
    double2 e = make_double2(0.0, 0.0);
    rc = apply_hamiltonian(h, lam, h->state, 0.0);
    if (!rc) rc = vec_dot(h, h->state, lam, h->namps, &e);
    if (!rc) rc = adjoint_walk(h, lam, K, grad);
    if (rc) return rc;
    *energy = e.x + h->ham.constant;
    return OVQE_OK;
}

extern "C" int ovqe_energy_gradient(ovqe_handle h, const double *theta, int32_t K, double *energy, double *grad) try {
    OVQE_ENTER(h);
    if (!h || !energy || !grad) return OVQE_ERR_INVALID;
    return energy_gradient_body(h, theta, K, energy, grad);
} OVQE_CATCH(h)

// ---- backward step of the adjoint method on a caller-held (psi, lambda) pair: plain handles and shard handles -------------
extern "C" int ovqe_adjoint_rotations(ovqe_handle h, void *lam_dev, int64_t R, const uint64_t *x, const uint64_t *z,
                                      const double *phi, double *w) try {
    OVQE_ENTER(h);
    if (!h || R < 0 || !lam_dev || (R && (!x || !z || !phi || !w))) return OVQE_ERR_INVALID;
    if (h->opt_real_state)
        return fail(h, OVQE_ERR_STATE, "ovqe_adjoint_rotations works on complex amplitudes: clear \"real_state\" and widen the buffer first");
    if (lam_dev == (void *)h->state) return fail(h, OVQE_ERR_STATE, "ovqe_adjoint_rotations: lam_dev is the state buffer");
    if (R == 0) return OVQE_OK;
    if (R >= (1ll << 30)) return fail(h, OVQE_ERR_INVALID, "too many rotations in one call");
    const uint64_t lmask = local_mask(h);
    const int ntot = h->n_local + h->n_global;
    const uint64_t allmask = ntot >= 64 ? ~0ull : ((1ull << ntot) - 1ull);
    for (int64_t r = 0; r < R; ++r) {
        if ((x[r] | z[r]) & ~allmask) return fail(h, OVQE_ERR_INVALID, "Pauli mask has bits beyond the register");
        if (x[r] & ~lmask)
            return fail(h, OVQE_ERR_INVALID,
                        "x mask touches global (rank) bits: exchange shards first (openvqe_amd/distributed.py)");
    }
    int rc = ensure_rp(h, (size_t)R);
    if (rc) return rc;
    for (int64_t r = 0; r < R; ++r) h->h_rp[r] = make_rot(x[r], z[r], phi[r]);
    HIPC(h, hipMemcpyAsync(h->d_rp.p, h->h_rp, (size_t)R * sizeof(RotParam), hipMemcpyHostToDevice, h->stream));
    // the op list of ovqe_apply_pauli_rotations (same-x runs), cut into tile segments for the BACKWARD kernel's tile size
    std::vector<SmallOp> ops;
    std::vector<SmallRot> rots((size_t)R);
    for (int64_t r0 = 0; r0 < R;) {
        int64_t r1 = r0 + 1;
        while (r1 < R && x[r1] == x[r0]) ++r1;
        SmallOp op = {};
        op.x = x[r0];
        op.kind = x[r0] ? OP_PAIR : OP_DIAG;
        op.first = (int32_t)r0;
        op.count = (int32_t)(r1 - r0);
        op.pivot = x[r0] ? 63 - __builtin_clzll(x[r0]) : 0;
        ops.push_back(op);
        for (int64_t r = r0; r < r1; ++r) rots[(size_t)r].z = z[r];
        r0 = r1;
    }
    TilePlan &tp = h->tp_adjoint;
    const int M = adjoint_tile_bits(h);
    if (M && ops.size() >= 2) {
        rc = build_tile_plan(h, ops, rots, std::vector<uint64_t>(ops.size(), 0), tp, false, M, tile_adj_rot_cap(M));
        if (rc) return rc;
    } else {
        tp.plan.assign(ops.size(), 0);
        for (size_t i = 0; i < ops.size(); ++i) tp.plan[i] = -1 - (int32_t)i;
    }
    // partial sums per workgroup and rotation: the streaming kernels as in ovqe_energy_gradient, the tile kernel one grid per CU set
    const int nb = (int)std::min<uint64_t>(65536, std::max<uint64_t>(1, (h->namps / 2 + 255) / 256));
    const int tgrid = M ? adjoint_tile_grid(h, M) : 0;
    rc = ensure(h, h->d_partials, std::max((size_t)ADJ_MAX_ROT * nb, (size_t)TILE_ROT_CAP * std::max(tgrid, 1)) * sizeof(double2));
    DevBuf d_w;
    if (!rc) rc = ensure(h, d_w, (size_t)R * sizeof(double));
    if (rc) return rc;
    amp_t *lam = (amp_t *)lam_dev;
    double *partials = (double *)h->d_partials.p;
    const RotParam *d_rp = (const RotParam *)h->d_rp.p;
    int64_t passes = 0;
    for (int si = (int)tp.plan.size() - 1; si >= 0 && !rc; --si) {
        const int32_t step = tp.plan[si];
        if (step >= 0) {
            const TileSeg &sg = tp.tsegs[step];
            rc = launch_tile_adjoint(h, lam, tp, sg, partials, tgrid);
            if (!rc)
                hipLaunchKernelGGL(k_reduce_rows, dim3(sg.rot1 - sg.rot0), dim3(256), 0, h->stream, (const double *)partials, tgrid,
                                   (double *)d_w.p + sg.rot0);
            ++passes;
            continue;
        }
        const SmallOp &op = ops[-1 - step];
        for (int hi = op.count; hi > 0; hi -= ADJ_MAX_ROT) {  // chunks from the end of the run backwards
            const int lo = std::max(0, hi - ADJ_MAX_ROT), cnt = hi - lo;
            if (op.kind == OP_PAIR)
                hipLaunchKernelGGL(k_adjoint_pairs, dim3(nb), dim3(256), 0, h->stream, h->state, lam, h->namps >> 1, op.pivot, op.x,
                                   h->base, d_rp + op.first + lo, cnt, partials);
            else
                hipLaunchKernelGGL(k_adjoint_diag, dim3(nb), dim3(256), 0, h->stream, h->state, lam, h->namps, h->base,
                                   d_rp + op.first + lo, cnt, partials);
            hipLaunchKernelGGL(k_reduce_rows, dim3(cnt), dim3(256), 0, h->stream, (const double *)partials, nb,
                               (double *)d_w.p + op.first + lo);
            ++passes;
        }
    }
    if (!rc && hipGetLastError() != hipSuccess) rc = fail(h, OVQE_ERR_HIP, "adjoint_rotations: launch failed");
    if (!rc && hipMemcpyAsync(w, d_w.p, (size_t)R * sizeof(double), hipMemcpyDeviceToHost, h->stream) != hipSuccess)
        rc = fail(h, OVQE_ERR_HIP, "adjoint_rotations: copy failed");
    if (hipStreamSynchronize(h->stream) != hipSuccess && !rc) rc = fail(h, OVQE_ERR_HIP, "adjoint_rotations: sync failed");
    if (d_w.p) (void)hipFree(d_w.p);
    if (rc) return rc;
    // the kernels sum Re (odd ny) / Im (even ny) of sum_i s_i conj(lam_i) psi_j; <lam|P|psi> carries i^ny on top
    for (int64_t r = 0; r < R; ++r)
        if (__builtin_popcountll(x[r] & z[r]) & 2) w[r] = -w[r];
    h->last_passes = passes;                                 // every pass reads and writes psi and lam once
    h->last_pass_bytes = (int64_t)(64.0 * (double)h->namps * (double)passes);
    return OVQE_OK;
} OVQE_CATCH(h)
