// hessian_host.inc — handle section of the exact energy Hessian (derivation and plan: sv_hessian_host.hpp; kernels: k_sparse_hessian in
// sv_sparse.hpp, sv_hessian.hpp; entry points: abi_hessian.inc).  Included by ovqe_sv.hip inside its anonymous namespace.
//
// Path 1: the metric's compact program (metric::build_compact: constant angles, offsets and first_op kept) with the Hamiltonian
// restricted to THAT program's compact indices, one launch of one wave per direction.  Path 2: two column stores and a backward walk of
// the op list.  Everything the call allocates is its own — the compact program included, a copy of this section's: no table of the
// energy paths or of the metric is touched.  The plan is cached per (program version, Hamiltonian version).

struct HessianDev {
    MetricDev *prog = nullptr;        // the compact program (only the program part of the record is used)
    hessian::Restricted R;            // of (plan_prog, plan_ham)
    int plan_prog = -1, plan_ham = -1;
    bool plan_ok = false;
    DevBuf d_theta, d_entries, d_out;          // path 1: rows [K * K], gradient [K], energy [1]
    DevBuf d_store, d_sigma, d_part, d_w;      // path 2
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    std::vector<double> host_out;
    int64_t info[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
};

void free_hessian(HessianDev *D) {
    if (!D) return;
    free_metric(D->prog);
    for (DevBuf *b : {&D->d_theta, &D->d_entries, &D->d_out, &D->d_store, &D->d_sigma, &D->d_part, &D->d_w})
        if (b->p) (void)hipFree(b->p);
    for (hipEvent_t e : D->ev)
        if (e) (void)hipEventDestroy(e);
    delete D;
}

// the compact program and the restricted Hamiltonian of (stored program, Hamiltonian in use), rebuilt when either changed
int hessian_plan(ovqe_handle h, HessianDev &D) {
    if (!D.prog) D.prog = new MetricDev();
    if (int rc = metric_compact(h, *D.prog)) return rc;
    if (D.plan_prog == h->prog_version && D.plan_ham == h->ham.version) return OVQE_OK;
    D.plan_prog = h->prog_version;
    D.plan_ham = h->ham.version;
    D.plan_ok = false;
    if (!D.prog->compact_ok) return OVQE_OK;
    if (!hessian::restrict_hamiltonian(D.prog->C.support, h->ham.groups, h->ham.terms, h->ham.constant, (size_t)16 << 20, &D.R)) return OVQE_OK;
    if (int rc = upload(h, D.d_entries, D.R.entries.data(), D.R.entries.size() * sizeof(hessian::Entry))) return rc;
    D.plan_ok = true;
    return OVQE_OK;
}

// the workspace behind its cap (workspace_cap, under the metric's option)
int hessian_cap(ovqe_handle h, size_t need, size_t held, bool fits, const char *what) {
    return workspace_cap(h, h->opt_metric_workspace_mb, need, held, fits, [&](size_t limit) {
        return std::string("ovqe_energy_hessian: ") + what + " need " + std::to_string(need) + " bytes, the cap is " + std::to_string(limit) +
               " bytes (option metric_workspace_mb)";
    });
}

// raw rows M -> (M + M^T) / 2, symmetric to the bit; returns max |M - M^T|
double hessian_symmetrise(const double *M, int K, double *hess) {
    double asym = 0.0;
    for (int i = 0; i < K; ++i)
        for (int j = i; j < K; ++j) {
            const double a = M[(size_t)i * K + j], b = M[(size_t)j * K + i];
            asym = std::max(asym, std::fabs(a - b));
            hess[(size_t)i * K + j] = hess[(size_t)j * K + i] = 0.5 * (a + b);
        }
    return asym;
}

int run_hessian_streaming(ovqe_handle h, HessianDev &D, const double *theta, double *energy, double *grad, double *hess, double *asymmetry);

int run_hessian(ovqe_handle h, const double *theta, double *energy, double *grad, double *hess, double *asymmetry) {
    const int K = h->K;
    if (!h->hessian) h->hessian = new HessianDev();
    HessianDev &D = *h->hessian;
    std::fill(D.info, D.info + 11, 0);
    int rc = ensure_events(h, D.ev, 4);
    if (rc) return rc;
    // ---- which form: the compact support when the program has one and the four vectors and the tables fit one workgroup's LDS
    int form = 0;
    SpHessArgs A = {};
    if (h->opt_force_path != 2) {
        if ((rc = hessian_plan(h, D))) return rc;
        if (D.plan_ok) {
            A = sp_hessian_args(D.prog->C, K, (int)D.R.entries.size(), D.R.constant);
            form = sp_hessian_lds(A, true).bytes <= LDS_WG_BUDGET ? 1 : sp_hessian_lds(A, false).bytes <= LDS_WG_BUDGET ? 2 : 0;
        }
    }
    if (!form) return run_hessian_streaming(h, D, theta, energy, grad, hess, asymmetry);
    const size_t nout = (size_t)K * K + (size_t)K + 1, out_bytes = nout * sizeof(double);
    const size_t work = out_bytes + D.R.entries.size() * sizeof(hessian::Entry);
    if ((rc = hessian_cap(h, work, D.d_out.cap + D.d_entries.cap, D.d_out.cap >= out_bytes, "the rows and the restricted Hamiltonian"))) return rc;
    if ((rc = ensure(h, D.d_out, out_bytes))) return rc;
    if ((rc = ensure(h, D.d_theta, (size_t)K * sizeof(double)))) return rc;
    const size_t lds = sp_hessian_lds(A, form == 1).bytes;
    const MetricDev &P = *D.prog;
    double *d_rows = (double *)D.d_out.p, *d_grad = d_rows + (size_t)K * K, *d_e = d_grad + K;
    HIPC(h, hipEventRecord(D.ev[0], h->stream));
    HIPC(h, hipMemcpyAsync(D.d_theta.p, theta, (size_t)K * sizeof(double), hipMemcpyHostToDevice, h->stream));
    rc = launch_staged<&k_sparse_hessian<true>, &k_sparse_hessian<false>>(
        h, form == 1, (unsigned)K, lds, A, (const double *)D.d_theta.p, (const metric::TabEntry *)P.d_tab.p, (const metric::Op *)P.d_ops.p,
        (const uint32_t *)P.d_pairs.p, (const int32_t *)P.d_first.p, (const SpEntry *)D.d_entries.p, d_rows, d_e, d_grad);
    if (rc) return rc;
    HIPC(h, hipEventRecord(D.ev[1], h->stream));
    D.host_out.resize(nout);
    HIPC(h, hipMemcpyAsync(D.host_out.data(), D.d_out.p, out_bytes, hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipEventRecord(D.ev[2], h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    const double asym = hessian_symmetrise(D.host_out.data(), K, hess);
    if (grad) std::copy(D.host_out.begin() + (size_t)K * K, D.host_out.begin() + (size_t)K * K + K, grad);
    if (energy) *energy = D.host_out[(size_t)K * K + K];
    if (asymmetry) *asymmetry = asym;
    D.info[0] = 1;
    D.info[1] = K;
    D.info[2] = A.m;
    D.info[3] = (int64_t)work;
    D.info[4] = 1;
    D.info[5] = A.nent;
    // [6] the copy of theta to the device and the launch, [7] the copy back; [8] stays 0: no third phase
    if ((rc = phases_us(h, D.ev, 2, D.info + 6))) return rc;
    D.info[9] = form;
    D.info[10] = (int64_t)lds;
    return OVQE_OK;
}

// ---- path 2 --------------------------------------------------------------------------------------------------------------------------
int run_hessian_streaming(ovqe_handle h, HessianDev &D, const double *theta, double *energy, double *grad, double *hess, double *asymmetry) {
    const int K = h->K, ncols = K + 1;
    const metric::Store st = metric::store_layout((int64_t)h->namps, K, false);
    // one weight record per parameterised rotation, record 0 the energy
    std::vector<int> rec_rot, rec_of(h->rots.size(), -1);
    for (size_t r = 0; r < h->rots.size(); ++r)
        if (h->rots[r].pidx >= 0 && h->rots[r].coeff != 0.0) {
            rec_of[r] = (int)rec_rot.size() + 1;
            rec_rot.push_back((int)r);
        }
    const size_t nrec = rec_rot.size() + 1;
    const hessian::Streaming W = hessian::streaming_layout((int64_t)h->namps, K, (int64_t)nrec);
    const uint64_t slab_rows = (uint64_t)W.slab_rows;
    const int nslabs = (int)W.nslabs;
    const size_t work = W.bytes;
    const bool fits = D.d_store.cap >= st.bytes && D.d_sigma.cap >= st.bytes && D.d_part.cap >= W.part_bytes && D.d_w.cap >= W.w_bytes;
    int rc = hessian_cap(h, work, D.d_store.cap + D.d_sigma.cap + D.d_part.cap + D.d_w.cap, fits,
                         "the two column stores, the slab sums and the weight records");
    if (rc) return rc;
    if ((rc = ensure(h, D.d_store, st.bytes))) return rc;
    if ((rc = ensure(h, D.d_sigma, st.bytes))) return rc;
    if ((rc = ensure(h, D.d_part, W.part_bytes))) return rc;
    if ((rc = ensure(h, D.d_w, W.w_bytes))) return rc;
    HIPC(h, hipMemsetAsync(D.d_store.p, 0, st.bytes, h->stream));
    HIPC(h, hipMemsetAsync(D.d_sigma.p, 0, st.bytes, h->stream));
    v2d *Av = (v2d *)D.d_store.p, *Sv = (v2d *)D.d_sigma.p;
    int64_t launches = 0;
    HIPC(h, hipEventRecord(D.ev[0], h->stream));
    // ---- the metric's tangent stage, then Sigma = H A: one launch per x-group over all columns
    if ((rc = metric_stream_tangents(h, D.d_store.p, st, theta, &launches, "ovqe_energy_hessian"))) return rc;
    const unsigned gy = (unsigned)((ncols + 63) / 64);
    const unsigned gx = (unsigned)std::min<uint64_t>((h->namps + 3) / 4, 65535u);
    for (const HGroup &g : h->ham.groups) {
        hipLaunchKernelGGL(k_hess_apply, dim3(gx, gy), dim3(256), 0, h->stream, (const v2d *)Av, Sv, h->namps, st.wpad, ncols, g.x,
                           (const HTerm *)h->ham.d_terms.p, g.t0, g.t1);
        HIPC(h, hipGetLastError());
        ++launches;
    }
    HIPC(h, hipEventRecord(D.ev[1], h->stream));
    // ---- the op list backwards on both stores
    auto weights = [&](size_t rec, uint64_t x, uint64_t z, int ny, int is_energy) -> int {
        hipLaunchKernelGGL(k_hess_weights, dim3((unsigned)nslabs, gy), dim3(256), 0, h->stream, (const v2d *)Av, (const v2d *)Sv, h->namps, slab_rows,
                           st.wpad, ncols, x, z, ny, is_energy, (double *)D.d_part.p);
        HIPC(h, hipGetLastError());
        hipLaunchKernelGGL(k_hess_weights_finish, dim3(gy), dim3(64), 0, h->stream, (const double *)D.d_part.p, nslabs, st.wpad, ncols,
                           (double *)D.d_w.p + rec * (size_t)st.wpad);
        HIPC(h, hipGetLastError());
        launches += 2;
        return OVQE_OK;
    };
    if ((rc = weights(0, 0, 0, 0, 1))) return rc;
    size_t met = 0;
    const unsigned ab = (unsigned)std::min<uint64_t>((h->namps + 255) / 256, 65535u);
    for (int oi = (int)h->ops.size() - 1; oi >= 0; --oi) {
        const SmallOp &op = h->ops[(size_t)oi];
        MetricSweep sw;   // (X, H and CNOT are their own inverses)
        if (!metric_sweep_of(op, &sw)) return fail(h, OVQE_ERR_INVALID, "ovqe_energy_hessian: internal: unexpected op in the sequential program");
        if (op.kind == OP_PAIR || op.kind == OP_DIAG) {
            for (int r = op.first + op.count - 1; r >= op.first; --r) {
                const SmallRot &sr = h->rots[(size_t)r];
                const bool param = sr.pidx >= 0 && sr.coeff != 0.0;
                const double phi = sr.phi0 + (sr.pidx >= 0 ? sr.coeff * theta[sr.pidx] : 0.0);
                if (param) {
                    if ((rc = weights((size_t)rec_of[(size_t)r], op.x, sr.z, sr.ny & 3, 0))) return rc;
                    ++met;
                }
                sw.kind = op.x ? MS_ROT : MS_DIAG;
                sw.z = sr.z;
                sw.ny = sr.ny & 3;
                sw.c = std::cos(phi);
                sw.s = -std::sin(phi);   // un-apply: the negated angle
                if ((rc = metric_sweep(h, Av, st, ncols, sw, &launches))) return rc;
                if ((rc = metric_sweep(h, Sv, st, ncols, sw, &launches))) return rc;
                if (!param) continue;
                for (v2d *V : {Av, Sv}) {   // column 1 + pidx += coeff (i P) column 0, of the un-applied states
                    hipLaunchKernelGGL(k_metric_add, dim3(ab), dim3(256), 0, h->stream, V, h->namps, st.wpad, sr.pidx + 1, op.x, sr.z, sr.ny & 3,
                                       -sr.coeff);
                    HIPC(h, hipGetLastError());
                    ++launches;
                }
            }
            continue;
        }
        if ((rc = metric_sweep(h, Av, st, ncols, sw, &launches))) return rc;
        if ((rc = metric_sweep(h, Sv, st, ncols, sw, &launches))) return rc;
    }
    if (met + 1 != nrec) return fail(h, OVQE_ERR_INVALID, "ovqe_energy_hessian: internal: the op list does not cover the rotations");
    HIPC(h, hipEventRecord(D.ev[2], h->stream));
    D.host_out.resize(nrec * (size_t)st.wpad);
    HIPC(h, hipMemcpyAsync(D.host_out.data(), D.d_w.p, D.host_out.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipEventRecord(D.ev[3], h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    // ---- rows: M[b][k] = sum over the rotations of parameter k of coeff 2 val[1 + b]; gradient: coeff val[0]
    std::vector<double> M((size_t)K * K, 0.0), g((size_t)K, 0.0);
    for (size_t q = 1; q < nrec; ++q) {
        const SmallRot &sr = h->rots[(size_t)rec_rot[q - 1]];
        const double *val = D.host_out.data() + q * (size_t)st.wpad;
        g[(size_t)sr.pidx] += sr.coeff * val[0];
        for (int b = 0; b < K; ++b) M[(size_t)b * K + sr.pidx] += 2.0 * sr.coeff * val[1 + b];
    }
    const double asym = hessian_symmetrise(M.data(), K, hess);
    if (grad) std::copy(g.begin(), g.end(), grad);
    if (energy) *energy = D.host_out[0] + h->ham.constant;
    if (asymmetry) *asymmetry = asym;
    D.info[0] = 2;
    D.info[1] = K;
    D.info[2] = (int64_t)h->namps;
    D.info[3] = (int64_t)work;
    D.info[4] = launches;
    D.info[5] = 0;
    if ((rc = phases_us(h, D.ev, 3, D.info + 6))) return rc;
    D.info[9] = 0;
    D.info[10] = 0;
    return OVQE_OK;
}
