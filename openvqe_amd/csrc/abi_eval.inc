// abi_eval.inc — C-ABI entry points, compiled evaluation: Hamiltonian and program upload, energy / energy_batch, sigma = H psi.
// Included by ovqe_sv.hip inside extern "C".

// ---- compiled evaluation ------------------------------------------------------------------------
int ovqe_set_hamiltonian(ovqe_handle h, int64_t T, const uint64_t *x, const uint64_t *z, const double *coeff,
                         double constant) try {
    OVQE_ENTER(h);
    if (!h || T < 0 || (T && (!x || !z || !coeff))) return OVQE_ERR_INVALID;
    int rc = install_hamdev(h, h->ham, T, x, z, coeff, constant);
    if (rc) return rc;
    free_sector(h->scr);   // the screen engine's tables belong to the Hamiltonian that was replaced
    h->scr_failed_version = -1;
    h->user_x.assign(x, x + T);
    h->user_z.assign(z, z + T);
    h->user_c.assign(coeff, coeff + T);
    h->user_const = constant;
    h->exp_lbits = -1;
    h->sp_tried = false;
    return install_conjugated_hamiltonian(h);
} OVQE_CATCH(h)

// energy-type entry points evaluate <phi|C^+ H C|phi> when the program's Clifford frame is open
struct FrameHamGuard {
    ovqe_handle h;
    bool on;
    explicit FrameHamGuard(ovqe_handle hh) : h(hh), on(hh && hh->frame_open && hh->ham_conj.set) {
        if (on) std::swap(h->ham, h->ham_conj);
    }
    ~FrameHamGuard() {
        if (on) std::swap(h->ham, h->ham_conj);
    }
};

int ovqe_set_program(ovqe_handle h, int64_t R, const uint64_t *x, const uint64_t *z, const double *coeff,
                     const double *phi0, const int32_t *pidx, int32_t K, uint64_t hf_index) try {
    OVQE_ENTER(h);
    if (h) h->prog_from_gates = false;
    if (h) h->forms_used = h->sp_forms = 0;
    if (h) std::fill(h->fused_launch, h->fused_launch + 6, 0);
    if (!h || R < 0 || K < 0 || (R && (!x || !z || !coeff || !pidx))) return OVQE_ERR_INVALID;
    const int ntot = h->n_local + h->n_global;
    const uint64_t allmask = ntot >= 64 ? ~0ull : ((1ull << ntot) - 1ull);
    if (hf_index & ~allmask) return fail(h, OVQE_ERR_INVALID, "hf_index out of range");
    for (int64_t r = 0; r < R; ++r) {
        if ((x[r] | z[r]) & ~allmask) return fail(h, OVQE_ERR_INVALID, "Pauli mask has bits beyond the register");
        if (x[r] & ~local_mask(h)) return fail(h, OVQE_ERR_INVALID, "x mask touches global (rank) bits");
        if (pidx[r] >= K) return fail(h, OVQE_ERR_INVALID, "parameter index >= K");
    }
    {   // does this list extend the previous one (see prev_x)?
        const size_t P = h->prev_x.size();
        bool ext = h->prog_set && P > 0 && (size_t)R >= P && h->prev_hf == hf_index;
        for (size_t r = 0; ext && r < P; ++r)
            ext = h->prev_x[r] == x[r] && h->prev_z[r] == z[r] && h->prev_coeff[r] == coeff[r] && h->prev_pidx[r] == pidx[r] &&
                  h->prev_phi0[r] == (phi0 ? phi0[r] : 0.0);
        h->prog_extends_prev = ext;
        h->prev_x.assign(x, x + R);
        h->prev_z.assign(z, z + R);
        h->prev_coeff.assign(coeff, coeff + R);
        h->prev_pidx.assign(pidx, pidx + R);
        h->prev_phi0.assign((size_t)R, 0.0);
        if (phi0) h->prev_phi0.assign(phi0, phi0 + R);
        h->prev_hf = hf_index;
    }
    h->prog_set = false;
    h->ops.clear();
    h->rots.clear();
    h->init_amp = make_double2(1.0, 0.0);
    h->K = K;
    h->hf = hf_index;
    h->frame_open = false;
    for (int64_t r = 0; r < R; ++r) push_rotation(h, x[r], z[r], coeff[r], phi0 ? phi0[r] : 0.0, pidx[r]);
    return finish_program(h);
} OVQE_CATCH(h)

int ovqe_set_gate_program(ovqe_handle h, int64_t G, const int32_t *opcode, const int32_t *b0, const int32_t *b1,
                          const double *ascale, const double *aconst, const int32_t *pidx, int32_t K,
                          uint64_t hf_index) try {
    OVQE_ENTER(h);
    if (!h || G < 0 || K < 0 || (G && (!opcode || !b0 || !b1 || !ascale || !aconst || !pidx))) return OVQE_ERR_INVALID;
    if (h->n_global) return fail(h, OVQE_ERR_INVALID, "gate programs are single-device");
    if (hf_index >> h->n_local) return fail(h, OVQE_ERR_INVALID, "hf_index out of range");
    for (int64_t g = 0; g < G; ++g) {
        if (b0[g] < 0 || b0[g] >= h->n_local) return fail(h, OVQE_ERR_INVALID, "gate bit out of range");
        if (opcode[g] == OVQE_GATE_CNOT && (b1[g] < 0 || b1[g] >= h->n_local || b1[g] == b0[g]))
            return fail(h, OVQE_ERR_INVALID, "CNOT target bit invalid");
        if (opcode[g] < 0 || opcode[g] > OVQE_GATE_CNOT) return fail(h, OVQE_ERR_INVALID, "unknown gate opcode");
        if (pidx[g] >= K) return fail(h, OVQE_ERR_INVALID, "parameter index >= K");
    }
    h->K = K;
    h->hf = hf_index;
    h->frame_open = false;
    h->prog_from_gates = false;
    h->prog_extends_prev = false;
    h->forms_used = h->sp_forms = 0;
    std::fill(h->fused_launch, h->fused_launch + 6, 0);
    h->prev_x.clear();
    if (h->opt_clifford_frame) {
        bool done = false;
        int rc = compile_gate_program_frame(h, G, opcode, b0, b1, ascale, aconst, pidx, &done);
        if (rc) return rc;
        if (done) {
            h->prog_from_gates = true;
            return OVQE_OK;
        }
    }
    return compile_gate_program_literal(h, G, opcode, b0, b1, ascale, aconst, pidx);
} OVQE_CATCH(h)

// the Clifford part of an open frame, literally, on the state in the buffer: |psi> = C |phi>
static int apply_tail_gates(ovqe_handle h) {
    int rc = OVQE_OK;
    for (size_t g = 0; g + 3 < h->tail_gates.size() && !rc; g += 4) {
        const int op = h->tail_gates[g], t = h->tail_gates[g + 1], c = h->tail_gates[g + 2];
        const double a = h->tail_gates[g + 3] > 0 ? M_PI_2 : -M_PI_2;
        rc = ovqe_apply_gate(h, op, t, c, a);
    }
    return rc;
}

int ovqe_prepare_state(ovqe_handle h, const double *theta, int32_t K) try {
    OVQE_ENTER(h);
    if (!h) return OVQE_ERR_INVALID;
    int rc = check_theta(h, theta, K);
    if (rc) return rc;
    rc = run_program_streaming(h, theta);
    if (rc || !h->frame_open) return rc;
    return apply_tail_gates(h);
} OVQE_CATCH(h)

// batched sector evaluations need the tables of the second sweep kernel (64-bit pair words) and the materialised <H>
static bool sector_batch_ready(ovqe_handle h) {
    const SectorEngine &E = h->sec;
    const bool real = h->opt_real_stream && h->prog_real_ok && h->n_global == 0 && tile_ok(h, true) && h->ham.groups.size() >= 3;
    return real && h->opt_sector && h->opt_sector_batch && E.valid && E.h_tables && E.pad_elems && !E.segs.empty() && E.segs[0].d_wide.p &&
           E.prog_version == h->prog_version && E.ham_version == h->ham.version &&
           sec_h_lds_bytes(std::max(E.h_max_tile, 1u), SEC_BATCH_NB, (uint32_t)E.h_max_dict) <= SEC_LDS_MAX;
}

int ovqe_energy_batch(ovqe_handle h, int64_t B, const double *theta, int32_t K, double *energies) try {
    OVQE_ENTER(h);
    if (!h || B < 0 || (B && !energies)) return OVQE_ERR_INVALID;
    FrameHamGuard frame_guard(h);
    int rc = check_theta(h, theta, K);
    if (rc) return rc;
    if (!h->ham.set) return fail(h, OVQE_ERR_STATE, "no Hamiltonian set (ovqe_set_hamiltonian)");
    if (B == 0) return OVQE_OK;
    if (h->opt_force_path == 0 || h->opt_force_path == 3) {
        // one wave owns an evaluation on the compact support: unbeatable for batches, but a lone evaluation of a
        // register beyond the LDS kernels is quicker on the whole chip (streaming + tiled sweeps) — and then the compact
        // program is not even built (an ADAPT ansatz at 24 qubits with a few thousand determinants: 20-100 ms of host work
        // per macro-iteration for tables no single evaluation would use)
        const bool wanted = h->opt_force_path == 3 || h->n_local <= 14 || B >= 16;
        if (wanted && !h->sp_tried) {
            rc = build_sparse_program(h);
            if (rc) return rc;
        }
        if (wanted && h->sp_valid) {
            bool done = false;
            rc = run_sparse(h, B, theta, energies, false, &done);
            if (rc || done) return rc;
        } else if (wanted) {
            h->sp_forms |= SPF_DECLINED;
        }
        if (h->opt_force_path == 3) return fail(h, OVQE_ERR_STATE, "program has no compact form (sparse path forced)");
    }
    if (use_small_path(h, B)) return run_small(h, B, theta, energies);
    // a lone evaluation is not timed with events (ovqe_last_batch_ms reads 0, as on the fused kernels' zero-copy path): every path below
    // ends with the host reading its result behind a synchronisation, and two event records + a second synchronisation + the
    // elapsed-time query are 6-8 us of the ~95 us of an ADAPT-sized evaluation
    const bool timed = B > 1;
    if (timed) HIPC(h, hipEventRecord(h->ev0, h->stream));
    auto lap_t = std::chrono::steady_clock::now();
    auto lap = [&](const char *what) {   // "sector_debug" bit 2 (value 4): stages of an evaluation that took more than 3 ms
        if (!(h->opt_sector_debug & 4)) return;
        const auto now = std::chrono::steady_clock::now();
        const double ms = std::chrono::duration<double, std::milli>(now - lap_t).count();
        if (ms > 3.0) fprintf(stderr, "ovqe: evaluation, %s: %.2f ms\n", what, ms);
        lap_t = now;
    };
    int64_t b_first = 0;
    if (B >= 4 && h->opt_sector_batch && h->opt_real_stream && h->prog_real_ok && h->n_global == 0 && tile_ok(h, true) &&
        h->ham.groups.size() >= 3) {
        rc = sector_prepare(h, true);   // a batch is worth the tables at once (a lone evaluation builds them at its second call)
        if (rc) return rc;
    }
    if (B >= 2 && sector_batch_ready(h)) {   // the whole batch in one pass of the sector tables
        bool ok = false;
        rc = run_sector_energy_batch(h, B, theta, false, energies, &ok);
        if (rc) return rc;
        if (ok) b_first = B;
    }
    for (int64_t b = b_first; b < B; ++b) {
        // programs that keep the amplitudes real stream 8 bytes per amplitude (state left as 2^n doubles)
        const bool real = h->opt_real_stream && h->prog_real_ok && h->n_global == 0 && tile_ok(h, true) &&
                          h->ham.groups.size() >= 3;
        if (real && h->ham_real.version != h->ham.version) {
            HamDev &R = h->ham_real;
            R.groups = h->ham.groups;
            R.terms = h->ham.terms;
            rc = upload(h, R.d_terms, R.terms.data(), R.terms.size() * sizeof(HTerm));
            if (rc) return rc;
            R.tile_bits = -1;
            R.version = h->ham.version;
        }
        if (real) {
            lap("before the sector tables");
            rc = sector_prepare(h);
            if (rc) return rc;
            lap("sector_prepare");
            SectorEngine &E = h->sec;
            if (E.valid && E.h_tables) {
                double2 res;
                bool ok = false;
                rc = run_sector_energy(h, theta + b * (int64_t)K, &res, &ok);
                if (rc) return rc;
                lap("run_sector_energy");
                if (ok) {
                    energies[b] = res.x + h->ham.constant;
                    continue;
                }
                sector_orphaned(h);   // a structurally-zero amplitude was not: these tables do not describe this program
            }
        }
        bool use_cc = false;
        if (real && h->opt_compact && h->n_local >= 18) {
            // compact cover: built at the second evaluation of a (program, Hamiltonian) pair — one-shot callers never pay
            HamDev &R = h->ham_real;
            CompactCover &C = h->cc;
            if (R.tile_bits != tile_bits(h, true) || R.tile_low != HAM_TILE_LOW || !R.tile_real) {
                rc = build_ham_tiles(h, R, true);
                if (rc) return rc;
            }
            if (C.prog_version != h->prog_version || C.ham_version != R.version || C.cover_id != R.cover_id) {
                C.valid = C.disabled = false;
                C.prog_version = h->prog_version;
                C.ham_version = R.version;
                C.cover_id = R.cover_id;
                C.seen = 0;
            }
            if (!C.valid && !C.disabled && ++C.seen >= 2) {
                rc = build_compact_cover(h, R);
                if (rc) return rc;
            }
            use_cc = C.valid;
        }
        if (use_cc && real && h->opt_sector && h->sec.valid && !h->sec.h_tables && h->sec.K == h->cc.K) {
            // circuit on the sector tables, <H> by the compact cover on the canonical compact state
            double2 res;
            bool ok = false;
            rc = run_sector_state(h, theta + b * (int64_t)K, (double *)h->cc.d_psic.p, &ok);
            if (rc) return rc;
            if (ok) {
                rc = run_expectation_compact(h, h->ham_real, &res, &ok, true);
                if (rc) return rc;
            }
            if (ok) {
                energies[b] = res.x + h->ham.constant;
                continue;
            }
            sector_orphaned(h);
        }
        lap("before the dense run");
        rc = run_program_streaming(h, theta + b * (int64_t)K, real);
        if (rc) return rc;
        lap("dense run");
        double2 res;
        bool tiled = false;
        if (use_cc) {
            rc = run_expectation_compact(h, h->ham_real, &res, &tiled);
            if (rc) return rc;
            if (!tiled) {  // the state left the recorded support: this program does not qualify
                h->cc.valid = false;
                h->cc.disabled = true;
            }
        }
        if (!tiled) rc = run_expectation_tiled(h, real ? h->ham_real : h->ham, &res, &tiled, real);
        if (rc) return rc;
        if (real && !tiled) return fail(h, OVQE_ERR_INVALID, "internal: real-amplitude path without a tile cover");
        if (!tiled)
            rc = run_bilinear(h, h->state, h->state, h->ham.groups, (const HGroup *)h->ham.d_groups.p,
                              (const HTerm *)h->ham.d_terms.p, &res, true);
        if (rc) return rc;
        lap("dense <H>");
        energies[b] = res.x + h->ham.constant;
    }
    if (!timed) {
        h->last_batch_ms = 0.f;
        return OVQE_OK;
    }
    HIPC(h, hipEventRecord(h->ev1, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    HIPC(h, hipEventElapsedTime(&h->last_batch_ms, h->ev0, h->ev1));
    return OVQE_OK;
} OVQE_CATCH(h)

int ovqe_energy_batch_device(ovqe_handle h, int64_t B, const void *theta_dev, int32_t K, void *energies_dev) try {
    OVQE_ENTER(h);
    if (!h || B < 0 || (B && (!theta_dev || !energies_dev))) return OVQE_ERR_INVALID;
    FrameHamGuard frame_guard(h);
    if (!h->prog_set) return fail(h, OVQE_ERR_STATE, "no program set (ovqe_set_program / ovqe_set_gate_program)");
    if (K != h->K || K <= 0) return fail(h, OVQE_ERR_INVALID, "K does not match the program's parameter count");
    if (!h->ham.set) return fail(h, OVQE_ERR_STATE, "no Hamiltonian set (ovqe_set_hamiltonian)");
    if (B == 0) return OVQE_OK;
    int rc;
    if (h->opt_force_path == 0 || h->opt_force_path == 3) {
        if (!h->sp_tried) {
            rc = build_sparse_program(h);
            if (rc) return rc;
        }
        if (h->sp_valid) {
            bool done = false;
            rc = run_sparse(h, B, (const double *)theta_dev, (double *)energies_dev, true, &done);
            if (rc || done) return rc;
        } else {
            h->sp_forms |= SPF_DECLINED;
        }
        if (h->opt_force_path == 3) return fail(h, OVQE_ERR_STATE, "program has no compact form (sparse path forced)");
    }
    if (h->n_global == 0 && h->n_local <= 16 && h->opt_force_path != 2)
        return run_small(h, B, (const double *)theta_dev, (double *)energies_dev, true);
    // larger registers: whole batches per pass of the sector tables, parameters and energies staying on the device
    if (h->opt_sector_batch && h->opt_real_stream && h->prog_real_ok && h->n_global == 0 && tile_ok(h, true) && h->ham.groups.size() >= 3) {
        rc = sector_prepare(h, true);
        if (rc) return rc;
        if (sector_batch_ready(h)) {
            bool ok = false;
            rc = run_sector_energy_batch(h, B, (const double *)theta_dev, true, (double *)energies_dev, &ok);
            if (rc) return rc;
            if (ok) return OVQE_OK;
        }
    }
    // anything else: through the host (one evaluation at a time on whatever path the program takes; B x K doubles down, B up)
    std::vector<double> th((size_t)B * K), en((size_t)B);
    HIPC(h, hipMemcpyAsync(th.data(), theta_dev, th.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    rc = ovqe_energy_batch(h, B, th.data(), K, en.data());
    if (rc) return rc;
    HIPC(h, hipMemcpyAsync(energies_dev, en.data(), en.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    return OVQE_OK;
} OVQE_CATCH(h)

int ovqe_energy(ovqe_handle h, const double *theta, int32_t K, double *energy) try {
    OVQE_ENTER(h);
    return ovqe_energy_batch(h, 1, theta, K, energy);
} OVQE_CATCH(h)

// Ascending list of the non-zero amplitudes of the state (d_nz_idx, d_nz_val) when they are at most 1/"screen_sparse" of the
// register; capacity: room for this many indices (0 = the support itself).
static int list_support(ovqe_handle h, uint64_t *support, bool *listed, uint64_t capacity) {
    *support = 0;
    *listed = false;
    if (h->opt_screen_sparse <= 0 || h->n_global != 0 || h->namps < 4096) return OVQE_OK;
    const uint64_t per_block = 256ull * NZ_PER_THREAD;
    const unsigned nbk = (unsigned)((h->namps + per_block - 1) / per_block);
    int rc = ensure(h, h->d_nz_cnt, (size_t)nbk * sizeof(uint32_t));
    if (!rc) rc = ensure(h, h->d_nz_start, (size_t)nbk * sizeof(uint64_t));
    if (rc) return rc;
    hipLaunchKernelGGL(k_nz_count, dim3(nbk), dim3(256), 0, h->stream, (const amp_t *)h->state, h->namps, (uint32_t *)h->d_nz_cnt.p);
    std::vector<uint32_t> cnt(nbk);
    hipError_t e = hipMemcpyAsync(cnt.data(), h->d_nz_cnt.p, (size_t)nbk * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail(h, OVQE_ERR_HIP, std::string("support list: ") + hipGetErrorString(e));
    std::vector<uint64_t> start(nbk);
    uint64_t total = 0;
    for (unsigned b = 0; b < nbk; ++b) {
        start[b] = total;
        total += cnt[b];
    }
    *support = total;
    if (total == 0 || total * (uint64_t)h->opt_screen_sparse > h->namps) return OVQE_OK;
    rc = upload(h, h->d_nz_start, start.data(), (size_t)nbk * sizeof(uint64_t));
    if (!rc) rc = ensure(h, h->d_nz_idx, std::max(total, capacity) * sizeof(uint64_t));
    if (!rc) rc = ensure(h, h->d_nz_val, total * sizeof(amp_t));
    if (rc) return rc;
    hipLaunchKernelGGL(k_nz_fill, dim3(nbk), dim3(256), 0, h->stream, (const amp_t *)h->state, h->namps,
                       (const uint64_t *)h->d_nz_start.p, (uint64_t *)h->d_nz_idx.p, (amp_t *)h->d_nz_val.p);
    HIPC(h, hipGetLastError());
    *listed = true;
    return OVQE_OK;
}

// ---- sigma = H psi of the ADAPT screens from the materialised Hamiltonian of psi's symmetry sector ----------------------------
// (ref:openvqe/adapt/fermionic_adapt_vqe.py:114 `sig = hamiltonian_sparse.dot(curr_state)`.)  An ADAPT state of a dozen operators
// lists 10^5 amplitudes, spread over every tile of the register: the tile cover then costs its 61 sweeps of the whole register
// (24 qubits: 24 ms) for a vector of 600 k numbers.  The sector — the closure of psi's support under the Hamiltonian's x-groups —
// does not change while the ansatz grows, so the restricted Hamiltonian is materialised ONCE per Hamiltonian (the row-format tables
// of the sector path, sector_host.inc build_sector_h, without a circuit) and sigma is one pass over it (k_sector_apply).  Real
// Hamiltonians and real states only; anything else takes the register path.
static int build_screen_sector(ovqe_handle h, uint64_t support) {
    SectorEngine &E = h->scr;
    free_sector(E);   // (before the build's block cache opens: sector_host.inc build_sector)
    DevBlockScope kept_blocks(h->kept_blocks);
    E.ham_version = h->ham.version;
    h->scr_failed_version = h->ham.version;   // until everything below succeeded
    if (h->n_global != 0 || h->n_local > 32 || h->n_local < 12) return OVQE_OK;
    for (const HTerm &t : h->ham.terms)
        if (t.ci != 0.0) return OVQE_OK;       // an odd number of Y with a real coefficient (or a complex one): sigma is not real
    for (const HGroup &g : h->ham.groups)
        if (g.x > 0xffffffffull) return OVQE_OK;
    // closure of the listed support under the x-groups (D_g(j) != 0, residues snapped): the symmetry sector psi lives in
    const uint64_t cap = h->namps / (uint64_t)std::max(h->opt_sector_sparsity, 2);
    if (support > cap) return OVQE_OK;
    DevBuf list, bitmap, total_b;
    struct Scratch {   // released on every way out (the HIPC macro returns from the middle)
        DevBuf &a, &b, &c;
        ~Scratch() {
            free_buf(a);
            free_buf(b);
            free_buf(c);
        }
    } scratch{list, bitmap, total_b};
    auto done = [&](int code) { return code; };
    const size_t words = (size_t)std::max<uint64_t>(1, h->namps >> 5);
    int rc = ensure(h, list, cap * sizeof(uint64_t));
    if (!rc) rc = ensure(h, bitmap, words * sizeof(uint32_t) + 16);
    if (!rc) rc = ensure(h, total_b, 256);
    if (rc) return done(rc == OVQE_ERR_ALLOC ? ((void)hipGetLastError(), OVQE_OK) : rc);
    HIPC(h, hipMemcpyAsync(list.p, h->d_nz_idx.p, support * sizeof(uint64_t), hipMemcpyDeviceToDevice, h->stream));
    HIPC(h, hipMemsetAsync(bitmap.p, 0, words * sizeof(uint32_t), h->stream));
    hipLaunchKernelGGL(k_support_mark, dim3((unsigned)((support + 255) / 256)), dim3(256), 0, h->stream, (const uint64_t *)list.p, support,
                       (uint32_t *)bitmap.p);
    unsigned long long total = support;
    HIPC(h, hipMemcpyAsync(total_b.p, &total, sizeof(total), hipMemcpyHostToDevice, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    uint64_t first = 0, last = support;
    for (int round = 0; round < 256 && last > first; ++round) {
        hipLaunchKernelGGL(k_support_expand, dim3((unsigned)((last - first + 255) / 256)), dim3(256), 0, h->stream, (uint64_t *)list.p, first,
                           last, cap, h->base, (const HGroup *)h->ham.d_groups.p, (int)h->ham.groups.size(),
                           (const HTerm *)h->ham.d_terms.p, (uint32_t *)bitmap.p, (unsigned long long *)total_b.p);
        HIPC(h, hipMemcpyAsync(&total, total_b.p, sizeof(total), hipMemcpyDeviceToHost, h->stream));
        HIPC(h, hipStreamSynchronize(h->stream));
        if (total > cap) return done(OVQE_OK);   // not a sparse sector
        first = last;
        last = total;
    }
    if (last > first || last > 0x7ffffff0ull) return done(OVQE_OK);
    const uint32_t K = (uint32_t)last;
    // ascending order (the sector path's canonical order), 32-bit indices
    DevBuf sorted;
    size_t tb = 0;
    hipError_t e = hipcub::DeviceRadixSort::SortKeys(nullptr, tb, (const uint64_t *)list.p, (uint64_t *)nullptr, (int)K, 0, h->n_local, h->stream);
    if (e != hipSuccess) return done(fail(h, OVQE_ERR_HIP, std::string("screen sector: sort (size query): ") + hipGetErrorString(e)));
    DevBuf temp;
    rc = ensure(h, sorted, (size_t)K * sizeof(uint64_t));
    if (!rc) rc = ensure(h, temp, tb);
    if (!rc) rc = ensure(h, E.d_sup, (size_t)K * sizeof(uint32_t));
    if (rc) {
        free_buf(sorted);
        free_buf(temp);
        return done(rc == OVQE_ERR_ALLOC ? ((void)hipGetLastError(), OVQE_OK) : rc);
    }
    tb = temp.cap;
    e = hipcub::DeviceRadixSort::SortKeys(temp.p, tb, (const uint64_t *)list.p, (uint64_t *)sorted.p, (int)K, 0, h->n_local, h->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_scr_narrow, dim3((K + 255u) / 256u), dim3(256), 0, h->stream, (const uint64_t *)sorted.p, K, (uint32_t *)E.d_sup.p);
        e = hipStreamSynchronize(h->stream);
    }
    free_buf(sorted);
    free_buf(temp);
    if (e != hipSuccess) return done(fail(h, OVQE_ERR_HIP, std::string("screen sector: sort: ") + hipGetErrorString(e)));
    free_buf(list);   // (the closure list: the largest of the three, not needed while the tables are built)
    E.K = K;
    E.M = sector_tile_bits(h);
    SectorScratch W;
    rc = ensure(h, W.inv_circ, (size_t)K * sizeof(uint32_t));
    if (rc) return rc == OVQE_ERR_ALLOC ? ((void)hipGetLastError(), OVQE_OK) : rc;
    hipLaunchKernelGGL(k_scr_iota, dim3((K + 255u) / 256u), dim3(256), 0, h->stream, (uint32_t *)W.inv_circ.p, K);
    size_t free_b = 0, total_mem = 0;
    HIPC(h, hipMemGetInfo(&free_b, &total_mem));
    const size_t budget = std::min<size_t>((size_t)std::max(h->opt_sector_max_gb, 0) << 30, free_b / 5 * 3);
    E.budget = budget;
    rc = build_sector_h(h, E, W, budget);
    if (rc == OVQE_ERR_ALLOC) {
        (void)hipGetLastError();
        free_sector(E);
        E.ham_version = h->ham.version;
        return OVQE_OK;
    }
    if (rc) return rc;
    if (!E.h_tables || E.hs.empty()) {
        free_sector(E);
        E.ham_version = h->ham.version;
        return OVQE_OK;
    }
    rc = ensure(h, E.d_buf[0], (size_t)K * sizeof(double));
    if (!rc) rc = ensure(h, E.d_buf[1], (size_t)K * sizeof(double));
    if (!rc) rc = ensure(h, E.d_flag, 256);
    if (rc) return rc;
    E.valid = true;
    h->scr_failed_version = -1;
    return OVQE_OK;
}
// sig (register) = (H + constant) psi through the screen engine; *used = false: the caller computes it on the register
static int screen_sector_sigma(ovqe_handle h, amp_t *sig, uint64_t support, bool *used) {
    *used = false;
    if (!h->opt_screen_sector || !h->opt_sector || h->n_global != 0 || support < (uint64_t)std::max(h->opt_screen_sector_min, 1)) return OVQE_OK;
    SectorEngine &E = h->scr;
    if (E.valid && E.ham_version != h->ham.version) free_sector(E);
    if (!E.valid) {
        if (h->scr_failed_version == h->ham.version) return OVQE_OK;
        int rc = build_screen_sector(h, support);
        if (rc) return rc;
        if (!E.valid) return OVQE_OK;
    }
    const uint32_t K = E.K;
    double *psic = (double *)E.d_buf[0].p, *sigc = (double *)E.d_buf[1].p;
    HIPC(h, hipMemsetAsync(psic, 0, (size_t)K * sizeof(double), h->stream));
    HIPC(h, hipMemsetAsync(E.d_flag.p, 0, sizeof(int), h->stream));
    hipLaunchKernelGGL(k_scr_compact, dim3((unsigned)((support + 255) / 256)), dim3(256), 0, h->stream, (const uint64_t *)h->d_nz_idx.p,
                       (const double2 *)h->d_nz_val.p, support, (const uint32_t *)E.d_sup.p, K, psic, (int *)E.d_flag.p);
    int flag = 0;
    HIPC(h, hipMemcpyAsync(&flag, E.d_flag.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    if (flag) return OVQE_OK;   // psi has left the sector the tables were built for, or is complex: register path (tables kept)
    int rc = sector_matvec(h, E, psic, sigc);
    if (rc) return rc;
    HIPC(h, hipMemsetAsync(sig, 0, h->namps * sizeof(amp_t), h->stream));
    hipLaunchKernelGGL(k_scr_scatter, dim3((K + 255u) / 256u), dim3(256), 0, h->stream, (double2 *)sig, (const uint32_t *)E.d_sup.p, K,
                       (const double *)sigc, (const double *)psic, h->ham.constant);
    HIPC(h, hipGetLastError());
    h->last_screen_sector = (int64_t)K;
    *used = true;
    return OVQE_OK;
}
