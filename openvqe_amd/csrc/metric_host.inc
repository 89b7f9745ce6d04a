// metric_host.inc — handle section of the Fubini-Study metric of the ansatz state (plan: sv_metric_host.hpp; kernels: k_sparse_metric in
// sv_sparse.hpp, sv_metric.hpp, and the Gram / finish kernels of sv_rdm.hpp; entry points: abi_metric.inc).  Included by ovqe_sv.hip
// inside its anonymous namespace.
//
// One call: the tangents T_k = d psi / d theta_k into an index-major store, then the Gram matrix of its columns (upper-triangular 64 x 64
// blocks, slabs summed in slice order, mirrored).  Everything the call allocates is its own: no table of the energy paths is touched and
// the state buffer is not used.  The host waits once, for the result.

struct MetricDev {
    DevBuf d_theta, d_tab, d_ops, d_pairs, d_first, d_store, d_slabs, d_out;
    metric::Compact C;
    int compact_version = -1;         // program version `C` was built for
    bool compact_ok = false;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    std::vector<double2> host_out;
    int64_t info[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
};

void free_metric(MetricDev *M) {
    if (!M) return;
    for (DevBuf *b : {&M->d_theta, &M->d_tab, &M->d_ops, &M->d_pairs, &M->d_first, &M->d_store, &M->d_slabs, &M->d_out})
        if (b->p) (void)hipFree(b->p);
    for (hipEvent_t e : M->ev)
        if (e) (void)hipEventDestroy(e);
    delete M;
}

// the metric's compact program of the stored program (sv_metric_host.hpp), rebuilt when the program changed
int metric_compact(ovqe_handle h, MetricDev &M) {
    if (M.compact_version == h->prog_version) return OVQE_OK;
    M.compact_version = h->prog_version;
    M.compact_ok = false;
    if (!h->opt_sparse || !h->opt_table_fusion || h->n_local > 40) return OVQE_OK;
    std::vector<metric::InOp> ops;
    std::vector<metric::InRot> rots;
    for (size_t o = 0; o < h->sops.size(); ++o) {
        const SmallOp &op = h->sops[o];
        ops.push_back(metric::InOp{op.x, h->sop_zc[o], op.kind, op.first, op.count});
    }
    for (const SmallRot &sr : h->srots) rots.push_back(metric::InRot{sr.z, sr.coeff, sr.phi0, sr.pidx, sr.ny});
    if (!metric::build_compact(h->hf, ops, rots, h->K, &M.C)) return OVQE_OK;
    int rc = upload(h, M.d_tab, M.C.tab.data(), M.C.tab.size() * sizeof(metric::TabEntry));
    if (!rc) rc = upload(h, M.d_ops, M.C.ops.data(), M.C.ops.size() * sizeof(metric::Op));
    if (!rc) rc = upload(h, M.d_pairs, M.C.pairs.data(), M.C.pairs.size() * sizeof(uint32_t));
    if (!rc) rc = upload(h, M.d_first, M.C.first_op.data(), M.C.first_op.size() * sizeof(int32_t));
    if (rc) return rc;
    HIPC(h, hipStreamSynchronize(h->stream));   // (the uploads read host vectors that the next rebuild replaces)
    M.compact_ok = true;
    return OVQE_OK;
}

// one op of the sequential program on psi and the live tangents (columns [0, ncols))
int metric_sweep(ovqe_handle h, void *store, const metric::Store &st, int ncols, const MetricSweep &S, int64_t *launches) {
    const uint64_t nwork = S.kind == MS_DIAG ? h->namps : h->namps >> 1;
    if (nwork == 0) return OVQE_OK;
    const unsigned gx = (unsigned)std::min<uint64_t>((nwork + 3) / 4, 65535u);
    const unsigned gy = (unsigned)((ncols + 63) / 64);
    hipLaunchKernelGGL(k_metric_sweep, dim3(gx, gy), dim3(256), 0, h->stream, (v2d *)store, nwork, st.wpad, ncols, S);
    HIPC(h, hipGetLastError());
    ++*launches;
    return OVQE_OK;
}

// the sweep of a literal op of the sequential program: x, the pivot, and for X / H / CNOT the kind (a rotation's kind, masks and angle
// are the caller's, rotation by rotation).  false: an op the sequential program cannot hold
bool metric_sweep_of(const SmallOp &op, MetricSweep *out) {
    MetricSweep sw = {};
    sw.x = op.x;
    sw.pivot = op.x ? 63 - __builtin_clzll(op.x) : 0;
    if (op.kind == OP_X) sw.kind = MS_X;
    else if (op.kind == OP_H) sw.kind = MS_H;
    else if (op.kind == OP_CNOT) {
        sw.kind = MS_CNOT;
        sw.ctrl = op.first;
    } else if (op.kind != OP_PAIR && op.kind != OP_DIAG) return false;
    *out = sw;
    return true;
}

// the streaming tangent stage: the sequential program once, every op on psi and the live tangents in one launch; behind a parameterised
// rotation its tangent takes coeff (-i P) psi.  O(K R) sweeps of the register.  `store` is zeroed by the caller; `who` names the entry point in an error text.
int metric_stream_tangents(ovqe_handle h, void *store, const metric::Store &st, const double *theta, int64_t *launches_out,
                           const char *who = "ovqe_metric_tensor") {
    int rc = OVQE_OK;
    int64_t launches = *launches_out;
    hipLaunchKernelGGL(k_metric_seed, dim3(1), dim3(64), 0, h->stream, (v2d *)store, h->hf, st.wpad);
    HIPC(h, hipGetLastError());
    int live = 1;   // columns in use: psi and the tangents of the parameters met so far
    const unsigned ab = (unsigned)std::min<uint64_t>((h->namps + 255) / 256, 65535u);
    for (const SmallOp &op : h->ops) {
        MetricSweep sw;
        if (!metric_sweep_of(op, &sw)) return fail(h, OVQE_ERR_INVALID, std::string(who) + ": internal: unexpected op in the sequential program");
        if (op.kind == OP_PAIR || op.kind == OP_DIAG) {
            for (int r = op.first; r < op.first + op.count; ++r) {
                const SmallRot &sr = h->rots[r];
                const double phi = sr.phi0 + (sr.pidx >= 0 ? sr.coeff * theta[sr.pidx] : 0.0);
                sw.kind = op.x ? MS_ROT : MS_DIAG;
                sw.z = sr.z;
                sw.ny = sr.ny & 3;
                sw.c = std::cos(phi);
                sw.s = std::sin(phi);
                if ((rc = metric_sweep(h, store, st, live, sw, &launches))) return rc;
                if (sr.pidx < 0 || sr.coeff == 0.0) continue;
                live = std::max(live, sr.pidx + 2);
                hipLaunchKernelGGL(k_metric_add, dim3(ab), dim3(256), 0, h->stream, (v2d *)store, h->namps, st.wpad, sr.pidx + 1, op.x, sr.z,
                                   sr.ny & 3, sr.coeff);
                HIPC(h, hipGetLastError());
                ++launches;
            }
            continue;
        }
        if ((rc = metric_sweep(h, store, st, live, sw, &launches))) return rc;
    }
    *launches_out = launches;
    return OVQE_OK;
}

int run_metric(ovqe_handle h, const double *theta, double *out) {
    const int K = h->K;
    if (!h->metric) h->metric = new MetricDev();
    MetricDev &M = *h->metric;
    std::fill(M.info, M.info + 11, 0);
    if (K == 0) return OVQE_OK;
    handle_num_cus(h);
    int rc = ensure_events(h, M.ev, 4);
    if (rc) return rc;
    // ---- which path: the compact support when the program has one and psi, one tangent and the tables fit one workgroup's LDS
    bool compact = false, stage = false;
    SpMetricArgs A = {};
    if (h->opt_force_path != 2) {
        if ((rc = metric_compact(h, M))) return rc;
        if (M.compact_ok) {
            A = sp_metric_args(M.C, K);
            compact = sp_metric_lds(A, false).bytes <= LDS_WG_BUDGET;
            stage = sp_metric_lds(A, true).bytes <= LDS_WG_BUDGET;
        }
    }
    const metric::Store st = metric::store_layout(compact ? (int64_t)M.C.m : (int64_t)h->namps, K, compact);
    // ---- the tangent store behind its cap
    rc = workspace_cap(h, h->opt_metric_workspace_mb, st.bytes, M.d_store.cap, M.d_store.cap >= st.bytes, [&](size_t limit) {
        return "ovqe_metric_tensor: the tangent store needs " + std::to_string(st.bytes) + " bytes (" + std::to_string(st.rows) +
               " amplitudes x " + std::to_string(st.wpad) + " columns), the cap is " + std::to_string(limit) + " bytes (option metric_workspace_mb)";
    });
    if (rc) return rc;
    const rdm::Schedule S = metric::gram_plan(st, h->num_cus);
    const size_t slab_bytes = S.slab_elems * S.elem_bytes;
    const int64_t W = st.width;
    if ((rc = ensure(h, M.d_store, st.bytes))) return rc;
    if ((rc = ensure(h, M.d_slabs, slab_bytes))) return rc;
    if ((rc = ensure(h, M.d_out, (size_t)W * W * sizeof(double2)))) return rc;
    if ((rc = ensure(h, M.d_theta, (size_t)K * sizeof(double)))) return rc;
    HIPC(h, hipMemsetAsync(M.d_store.p, 0, st.bytes, h->stream));   // (the padding columns of the Gram blocks read as zeros)
    HIPC(h, hipMemsetAsync(M.d_slabs.p, 0, slab_bytes, h->stream));
    int64_t launches = 0;
    size_t tangent_lds = 0;
    HIPC(h, hipEventRecord(M.ev[0], h->stream));
    if (compact) {
        A.wpad = st.wpad;
        tangent_lds = sp_metric_lds(A, stage).bytes;
        HIPC(h, hipMemcpyAsync(M.d_theta.p, theta, (size_t)K * sizeof(double), hipMemcpyHostToDevice, h->stream));
        rc = launch_staged<&k_sparse_metric<true>, &k_sparse_metric<false>>(
            h, stage, (unsigned)K, tangent_lds, A, (const double *)M.d_theta.p, (const metric::TabEntry *)M.d_tab.p, (const metric::Op *)M.d_ops.p,
            (const uint32_t *)M.d_pairs.p, (const int32_t *)M.d_first.p, (double *)M.d_store.p);
        if (rc) return rc;
        launches = 1;
    } else {
        if ((rc = metric_stream_tangents(h, M.d_store.p, st, theta, &launches))) return rc;
    }
    HIPC(h, hipEventRecord(M.ev[1], h->stream));
    // ---- Gram matrix of the store's columns: the density matrices' kernels on the index-major store
    constexpr RdmGramLds GL = rdm_gram_lds();
    const unsigned gb = (unsigned)(S.npairs * S.slices), fb = (unsigned)(((uint64_t)W * W + 255) / 256);
    if (compact) {
        hipLaunchKernelGGL(k_rdm_gram<true>, dim3(gb), dim3(rdm::GRAM_THREADS), GL.bytes, h->stream, (const void *)M.d_store.p, st.rows, st.wpad, S.nblk,
                           S.slices, S.slice_rows, M.d_slabs.p);
        HIPC(h, hipGetLastError());
        HIPC(h, hipEventRecord(M.ev[2], h->stream));
        hipLaunchKernelGGL(k_rdm_finish<true>, dim3(fb), dim3(256), 0, h->stream, (const void *)M.d_slabs.p, W, S.nblk, S.slices, (double2 *)M.d_out.p);
    } else {
        hipLaunchKernelGGL(k_rdm_gram<false>, dim3(gb), dim3(rdm::GRAM_THREADS), GL.bytes, h->stream, (const void *)M.d_store.p, st.rows, st.wpad, S.nblk,
                           S.slices, S.slice_rows, M.d_slabs.p);
        HIPC(h, hipGetLastError());
        HIPC(h, hipEventRecord(M.ev[2], h->stream));
        hipLaunchKernelGGL(k_rdm_finish<false>, dim3(fb), dim3(256), 0, h->stream, (const void *)M.d_slabs.p, W, S.nblk, S.slices, (double2 *)M.d_out.p);
    }
    HIPC(h, hipGetLastError());
    HIPC(h, hipEventRecord(M.ev[3], h->stream));
    M.host_out.resize((size_t)W * W);
    HIPC(h, hipMemcpyAsync(M.host_out.data(), M.d_out.p, (size_t)W * W * sizeof(double2), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    // ---- g.  Compact support: <psi|T_k> = 0 on a real state, g is the Gram matrix.  Streaming: column 0 of the Gram matrix is
    // a_k = <T_k|psi>, and g_ij = Re G_ij - Re(a_i conj(a_j)); upper triangle, mirrored: symmetric to the bit either way
    const double2 *G = M.host_out.data();
    for (int i = 0; i < K; ++i)
        for (int j = i; j < K; ++j) {
            double g;
            if (compact) {
                g = G[(size_t)i * W + j].x;
            } else {
                const double2 ai = G[(size_t)(i + 1) * W], aj = G[(size_t)(j + 1) * W];
                g = G[(size_t)(i + 1) * W + (j + 1)].x - (ai.x * aj.x + ai.y * aj.y);
            }
            out[(size_t)i * K + j] = out[(size_t)j * K + i] = g;
        }
    M.info[0] = compact ? 1 : 2;
    M.info[1] = K;
    M.info[2] = st.rows;
    M.info[3] = (int64_t)st.bytes;
    M.info[4] = launches;
    M.info[5] = 1;
    if ((rc = phases_us(h, M.ev, 3, M.info + 6))) return rc;
    M.info[9] = compact ? (stage ? 1 : 2) : 0;
    M.info[10] = (int64_t)tangent_lds;
    return OVQE_OK;
}
