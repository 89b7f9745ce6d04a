// gradbatch_host.inc — handle section of the batched exact gradient (geometry: sv_gradbatch_host.hpp; kernel: k_sparse_grad_batch in
// sv_sparse.hpp; entry points: abi_gradbatch.inc), and what the four batched cost functions on the compact support share — this one,
// deflate_host.inc, spread_host.inc, constrain_host.inc: the decision for path 1 (compact_batch_plan), what a call owns (BatchIo), the
// launch (for_batch_waves, launch_compact_batch), and what their entry points share (batch_refusals, overlaps_out, info_out).
// Included by ovqe_sv.hip inside its anonymous namespace.
//
// Path 1: the handle's compact program as run_sparse_gradient uses it (d_sp_ops, d_sp_pairs, d_rots, d_sp_entries), the whole batch in
// one launch.  Nothing is planned or built here beyond what the single call builds on its first use.  Everything the call allocates is
// this record's: h->d_theta, the mapped I/O slot and sp_forms are not touched.  Path 2 (every other program): abi_gradbatch.inc runs
// the single call's body row by row.

static_assert(gradbatch::LDS_BUDGET == LDS_WG_BUDGET && gradbatch::LDS_CU == LDS_WG_MAX, "sv_gradbatch_host.hpp plans with this file's budgets");

// Whether a batch of B rows runs on the compact support, with the kernel arguments and the launch geometry: ONE decision for the four
// calls (ovqe_spread_gradient_batch asks more of the program behind it).  *ok = false: not eligible (nothing was launched).
int compact_batch_plan(ovqe_handle h, int64_t B, SparseArgs *args, gradbatch::Plan *plan, bool *ok) {
    *ok = false;
    if (!(h->opt_force_path == 0 || h->opt_force_path == 3) || !h->opt_sparse_grad || h->n_local > 16) return OVQE_OK;
    int rc = OVQE_OK;
    if (!h->sp_tried && (rc = build_sparse_program(h))) return rc;
    if (!h->sp_valid) return OVQE_OK;
    const SparseArgs A = sparse_args(h, B);
    if (!gradbatch::eligible(A)) return OVQE_OK;
    const gradbatch::Plan G = gradbatch::plan(A, B, h->opt_grad_batch_waves, h->opt_grad_batch_workgroups, handle_num_cus(h));
    if (!G.ok) return OVQE_OK;
    *args = A;
    *plan = G;
    *ok = true;
    return OVQE_OK;
}

// What every path-1 call owns: the rows on the device, the results, and the events around upload | launch | download.
struct BatchIo {
    DevBuf d_theta, d_out;   // rows [B * K]; the call's results (each record says which)
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    void release() {
        for (DevBuf *b : {&d_theta, &d_out})
            if (b->p) (void)hipFree(b->p);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    // room for the rows and `out` doubles of results; event 0, then the rows on their way up
    int begin(ovqe_handle h, const double *theta, size_t rows, size_t out) {
        int rc = ensure_events(h, ev, 3);
        if (!rc) rc = ensure(h, d_theta, rows * sizeof(double));
        if (!rc) rc = ensure(h, d_out, out * sizeof(double));
        if (rc) return rc;
        HIPC(h, hipEventRecord(ev[0], h->stream));
        HIPC(h, hipMemcpyAsync(d_theta.p, theta, rows * sizeof(double), hipMemcpyHostToDevice, h->stream));
        return OVQE_OK;
    }
    // event 2 behind the copies back, the stream drained; phase_us[0 .. 1]: upload + launch, download
    int end(ovqe_handle h, int64_t *phase_us) {
        HIPC(h, hipEventRecord(ev[2], h->stream));
        HIPC(h, hipStreamSynchronize(h->stream));
        return phases_us(h, ev, 2, phase_us);
    }
};

// the planned number of waves as a compile-time constant: launch(std::integral_constant<int, NW>())
template <class Launch>
int for_batch_waves(int nw, Launch launch) {
    switch (nw) {
    case 1: return launch(std::integral_constant<int, 1>());
    case 2: return launch(std::integral_constant<int, 2>());
    case 4: return launch(std::integral_constant<int, 4>());
    default: return launch(std::integral_constant<int, 8>());
    }
}
// a batch kernel of sv_sparse.hpp in its staged or plain instance on the planned geometry: the arguments the four share, then its own;
// event 1 behind it
template <auto Staged, auto Plain, class... Own>
int launch_compact_batch(ovqe_handle h, const gradbatch::Plan &G, const SparseArgs &A, const BatchIo &io, Own... own) {
    if (int rc = lds_opt_in<Staged, Plain>(h, LDS_WG_MAX)) return rc;
    hipLaunchKernelGGL(G.stage ? Staged : Plain, dim3((unsigned)G.workgroups), dim3((unsigned)G.nw * 64), G.lds, h->stream, A,
                       (const double *)io.d_theta.p, (const SmallRot *)h->d_rots.p, (const SpOp *)h->d_sp_ops.p,
                       (const uint32_t *)h->d_sp_pairs.p, (const SpEntry *)h->d_sp_entries.p, own...);
    HIPC(h, hipGetLastError());
    HIPC(h, hipEventRecord(io.ev[1], h->stream));
    return OVQE_OK;
}

struct GradBatchDev {
    BatchIo io;   // results: energies [B], then gradients [B * K]
    int64_t info[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
};

void free_grad_batch(GradBatchDev *D) {
    if (!D) return;
    D->io.release();
    delete D;
}

// *done = false: the program is not eligible for path 1 (nothing was launched, info untouched)
int run_grad_batch(ovqe_handle h, int64_t B, const double *theta, double *energies, double *grads, bool *done) {
    *done = false;
    int rc = OVQE_OK;
    SparseArgs A;
    gradbatch::Plan G;
    bool ok = false;
    if ((rc = compact_batch_plan(h, B, &A, &G, &ok)) || !ok) return rc;
    if (!h->grad_batch) h->grad_batch = new GradBatchDev();
    GradBatchDev &D = *h->grad_batch;
    const size_t K = (size_t)h->K, rows = (size_t)B * K;
    if ((rc = D.io.begin(h, theta, rows, (size_t)B + rows))) return rc;
    double *d_e = (double *)D.io.d_out.p, *d_g = d_e + B;
    rc = for_batch_waves(G.nw, [&](auto NW) {
        constexpr int nw = decltype(NW)::value;
        return launch_compact_batch<&k_sparse_grad_batch<nw, true>, &k_sparse_grad_batch<nw, false>>(h, G, A, D.io, d_e, d_g);
    });
    if (rc) return rc;
    HIPC(h, hipMemcpyAsync(energies, d_e, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipMemcpyAsync(grads, d_g, rows * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    const int64_t info[9] = {1, B, (int64_t)K, 1, G.stage ? 1 : 2, G.nw, G.workgroups, (int64_t)G.lds, h->sp_m};
    if ((rc = D.io.end(h, D.info + 9))) return rc;
    std::copy(info, info + 9, D.info);
    *done = true;
    return OVQE_OK;
}

// ---- what the entry points of the four calls share (abi_gradbatch.inc, abi_deflate.inc, abi_spread.inc, abi_constrain.inc) ----------

// The refusals of ovqe_*_gradient_batch, in the ONE order they fire: B negative; what ovqe_energy_gradient refuses, with its codes
// (no program, K, no Hamiltonian, a shard handle); option real_state where the call refuses it; own() — the checks of the call's
// own arguments; an open Clifford frame where the call refuses it; B = 0 (*empty = true: the call returns OVQE_OK with nothing
// written); the NULL pointers; the range of B x K.
struct BatchCall {
    const char *fn;            // the entry point's name, for the messages
    bool real_state;           // refused under option real_state
    const char *frame_lives;   // null, or what lives in the caller's frame: the call is refused while the Clifford frame is open
    const char *out_name;      // the result that must not be NULL ...
    const void *out;           // ... and its pointer
};
template <class Own>
int batch_refusals(ovqe_handle h, const BatchCall &C, int64_t B, const double *theta, int32_t K, const double *grads, bool *empty, Own own) {
    const std::string fn = C.fn;
    *empty = false;
    if (B < 0) return fail(h, OVQE_ERR_INVALID, fn + ": B is negative");
    if (!h->prog_set) return fail(h, OVQE_ERR_STATE, "no program set (ovqe_set_program / ovqe_set_gate_program)");
    if (K != h->K) return fail(h, OVQE_ERR_INVALID, "K does not match the program's parameter count");
    if (!h->ham.set) return fail(h, OVQE_ERR_STATE, "no Hamiltonian set (ovqe_set_hamiltonian)");
    if (h->n_global) return fail(h, OVQE_ERR_INVALID, fn + " is single-device, as ovqe_energy_gradient: not available on a shard handle");
    if (C.real_state && h->opt_real_state)
        return fail(h, OVQE_ERR_STATE, fn + ": not available under option real_state (the buffer holds 8-byte amplitudes)");
    if (int rc = own()) return rc;
    if (C.frame_lives && h->frame_open)
        return fail(h, OVQE_ERR_STATE, fn + ": the gate program's Clifford frame is open — " + C.frame_lives +
                                           " in the caller's frame, the evaluated state does not; option \"clifford_frame\" = 0 runs such a list literally");
    if (B == 0) {
        *empty = true;
        return OVQE_OK;
    }
    if (!C.out) return fail(h, OVQE_ERR_INVALID, fn + ": " + C.out_name + " is NULL");
    if (K > 0 && (!theta || !grads)) return fail(h, OVQE_ERR_INVALID, fn + ": " + (theta ? "grads" : "theta") + " is NULL");
    if (B > ((int64_t)1 << 40) / std::max<int64_t>(K, 1)) return fail(h, OVQE_ERR_INVALID, fn + ": B x K is out of range");
    return OVQE_OK;
}
int batch_refusals(ovqe_handle h, const BatchCall &C, int64_t B, const double *theta, int32_t K, const double *grads, bool *empty) {
    return batch_refusals(h, C, B, theta, K, grads, empty, [] { return (int)OVQE_OK; });   // (a call with no checks of its own)
}

// row b of overlaps_re_im [B x J x 2] from the streaming path's o[J]
void overlaps_out(double *overlaps_re_im, int64_t b, int64_t J, const double2 *o) {
    for (int64_t j = 0; j < J; ++j) {
        overlaps_re_im[2 * (b * J + j)] = o[j].x;
        overlaps_re_im[2 * (b * J + j) + 1] = o[j].y;
    }
}

// behind the four *_info getters: the first min(count, n) of a section's info values; zeros where the section has not run (src null)
int info_out(ovqe_handle h, const int64_t *src, int n, int64_t *info, int count) {
    if (!h || !info || count < 0) return OVQE_ERR_INVALID;
    for (int i = 0; i < count && i < n; ++i) info[i] = src ? src[i] : 0;
    return OVQE_OK;
}
