// gates_host.inc — literal gate programs: small-gate lowering, the Clifford-frame compilation into Pauli rotations (sv_frame_host.hpp) and
// the op lists the streaming / tile paths consume.  Included by ovqe_sv.hip inside its anonymous namespace.

// ---- gate programs ---------------------------------------------------------------------------------
void push_gate(ovqe_handle h, int opcode, int b0, int b1) {
    SmallOp op = {};
    if (opcode == OVQE_GATE_CNOT) {
        op.x = 1ull << b1;
        op.kind = OP_CNOT;
        op.first = b0;
        op.count = b1;
        op.pivot = b1;
    } else {
        op.x = 1ull << b0;
        op.kind = opcode == OVQE_GATE_X ? OP_X : OP_H;
        op.pivot = b0;
    }
    h->ops.push_back(op);
}

void push_literal_gate(ovqe_handle h, int opcode, int b0, int b1, double ascale, double aconst, int32_t pidx) {
    const uint64_t bit = 1ull << b0;
    switch (opcode) {
    case OVQE_GATE_RX: push_rotation(h, bit, 0, 0.5 * ascale, 0.5 * aconst, pidx); break;
    case OVQE_GATE_RY: push_rotation(h, bit, bit, 0.5 * ascale, 0.5 * aconst, pidx); break;
    case OVQE_GATE_RZ: push_rotation(h, 0, bit, 0.5 * ascale, 0.5 * aconst, pidx); break;
    default: push_gate(h, opcode, b0, b1);
    }
}

// the literal gate list, one op per gate (consecutive rotations with equal x masks still share a sweep)
int compile_gate_program_literal(ovqe_handle h, int64_t G, const int32_t *opcode, const int32_t *b0, const int32_t *b1,
                                 const double *ascale, const double *aconst, const int32_t *pidx) {
    h->prog_set = false;
    h->ops.clear();
    h->rots.clear();
    h->init_amp = make_double2(1.0, 0.0);
    for (int64_t g = 0; g < G; ++g) push_literal_gate(h, opcode[g], b0[g], b1[g], ascale[g], aconst[g], pidx[g]);
    return finish_program(h);
}

// Clifford-frame compilation.  X, H, CNOT and the fixed quarter-turn rotations RX/RY/RZ(+-pi/2) of the reference's
// templates (ref:openvqe/common_files/circuit.py:13-106) are Clifford gates: with C_<k the product of the Clifford
// gates before rotation k,   U = C_total * prod_k exp(-i phi_k C_<k^dagger P_k C_<k),   and the conjugated generator
// is again a Pauli string (Heisenberg picture; tracked as images of X_q, Z_q).  When C_total is the identity — every
// QUCCSD template returns the frame to the identity: its Clifford part only routes the excitation — the literal gate
// list is EXACTLY a sequence of Pauli rotations, which then take the fused same-x / commuting-run / real-mode /
// support-compacted paths.  C_total = e^{i alpha}: the phase is read from one execution of the Clifford part alone
// on |hf>; anything but alpha = 0 (or a frame that does not close) keeps the literal program.
// clifford_frame = 2 (tests): always use the frame form and append the Clifford part literally.

int install_hamdev(ovqe_handle h, HamDev &H, int64_t T, const uint64_t *x, const uint64_t *z, const double *coeff, double constant) {
    H.set = false;
    int rc = build_groups(h, T, x, z, coeff, nullptr, false, H.groups, H.terms);
    if (rc) return rc;
    rc = upload(h, H.d_groups, H.groups.data(), H.groups.size() * sizeof(HGroup));
    if (!rc) rc = upload(h, H.d_terms, H.terms.data(), H.terms.size() * sizeof(HTerm));
    if (rc) return rc;
    H.constant = constant;
    H.set = true;
    H.tile_bits = -1;  // tile cover rebuilt on first use
    H.version = ++h->ham_versions;
    return OVQE_OK;
}

// stored Hamiltonian through the open Clifford frame: P = i^{|x&z|} X^x Z^z -> product of the images of its X_q and Z_q
int install_conjugated_hamiltonian(ovqe_handle h) {
    h->ham_conj.set = false;
    if (!h->frame_open || !h->ham.set) return OVQE_OK;
    const int n = h->n_local;
    const size_t T = h->user_x.size();
    std::vector<uint64_t> cx(T), cz(T);
    std::vector<double> cc(T);
    auto img = [&](int idx) { return PauliRaw{h->frame_img[3 * idx], h->frame_img[3 * idx + 1], (int)h->frame_img[3 * idx + 2]}; };
    for (size_t t = 0; t < T; ++t) {
        const uint64_t x = h->user_x[t], z = h->user_z[t];
        PauliRaw acc{0, 0, __builtin_popcountll(x & z) & 3};   // the i^{|x&z|} of the Hermitian string
        for (int q = 0; q < n; ++q)
            if ((x >> q) & 1) acc = pauli_mul(acc, img(q));
        for (int q = 0; q < n; ++q)
            if ((z >> q) & 1) acc = pauli_mul(acc, img(n + q));
        const int rel = (acc.k - __builtin_popcountll(acc.x & acc.z)) & 3;
        if (rel & 1) return fail(h, OVQE_ERR_INVALID, "internal: non-Hermitian conjugated Hamiltonian term");
        cx[t] = acc.x;
        cz[t] = acc.z;
        cc[t] = rel ? -h->user_c[t] : h->user_c[t];
    }
    return install_hamdev(h, h->ham_conj, (int64_t)T, cx.data(), cz.data(), cc.data(), h->user_const);
}

int compile_gate_program_frame(ovqe_handle h, int64_t G, const int32_t *opcode, const int32_t *b0, const int32_t *b1,
                               const double *ascale, const double *aconst, const int32_t *pidx, bool *done) {
    *done = false;
    const int n = h->n_local;
    FrameTrack F;
    if (!track_clifford_frame(n, G, opcode, b0, b1, ascale, aconst, pidx, F))
        return fail(h, OVQE_ERR_INVALID, "internal: non-Hermitian conjugated generator");
    std::vector<PauliRaw> &ix = F.ix, &iz = F.iz;
    std::vector<FrameEmit> &emitted = F.emitted;
    std::vector<int64_t> &tail = F.tail;  // gates folded into the frame (the Clifford part, original order)
    const bool closed = F.closed;
    const bool forced = h->opt_clifford_frame == 2;
    if (!closed && !forced) {
        // Open frame (e.g. interleaved CNOT ladders, which the reference's ladder code does not undo): the program is the
        // rotation sequence; the net Clifford operator goes into the Hamiltonian for energies (install_conjugated_hamiltonian)
        // and behind the rotations, gate by gate, for ovqe_prepare_state.  Option 3 keeps the literal program instead.
        if (h->opt_clifford_frame == 3 || n > 63) return OVQE_OK;
        h->prog_set = false;
        h->ops.clear();
        h->rots.clear();
        h->init_amp = make_double2(1.0, 0.0);
        for (const FrameEmit &e : emitted) push_rotation(h, e.x, e.z, e.coeff, e.phi0, e.pidx);
        h->frame_img.assign((size_t)6 * n, 0);
        for (int q = 0; q < n; ++q) {
            h->frame_img[3 * q] = ix[q].x;
            h->frame_img[3 * q + 1] = ix[q].z;
            h->frame_img[3 * q + 2] = (uint64_t)ix[q].k;
            h->frame_img[3 * (n + q)] = iz[q].x;
            h->frame_img[3 * (n + q) + 1] = iz[q].z;
            h->frame_img[3 * (n + q) + 2] = (uint64_t)iz[q].k;
        }
        h->tail_gates.clear();
        for (const int64_t g : tail) {
            h->tail_gates.push_back(opcode[g]);
            h->tail_gates.push_back(b0[g]);
            h->tail_gates.push_back(b1[g]);
            h->tail_gates.push_back(aconst[g] > 0 ? 1 : -1);
        }
        h->frame_open = true;
        *done = true;
        int rc = finish_program(h);
        if (!rc) rc = install_conjugated_hamiltonian(h);
        if (rc) h->frame_open = false;
        return rc;
    }
    bool drop_tail = false;
    double2 phase = make_double2(1.0, 0.0);
    h->init_amp = phase;
    if (closed && !forced) {
        // global phase of the Clifford part: execute it alone on |hf>
        h->prog_set = false;
        h->ops.clear();
        h->rots.clear();
        double2 amp = make_double2(0.0, 0.0);
        std::complex<double> amp_host(0.0, 0.0);
        const bool on_host = !tail.empty() && h->opt_clifford_phase_host && n <= 63 &&
                             clifford_amplitude_on_host(h->hf, tail, opcode, b0, b1, aconst, &amp_host);
        if (on_host) amp = make_double2(amp_host.real(), amp_host.imag());
        if (!tail.empty() && !on_host)
            for (const int64_t g : tail) push_literal_gate(h, opcode[g], b0[g], b1[g], ascale[g], aconst[g], pidx[g]);
        if (!tail.empty()) {
            // (device form) the Clifford part is installed as the handle's program only for this one execution: whatever happens
            // below, the handle must not keep reporting it as a valid program (prog_set stays false until the final
            // program is installed by the last finish_program)
            int rc = OVQE_OK;
            if (!on_host) {
                rc = finish_program(h);
                if (!rc) {
                    std::vector<double> zero((size_t)std::max(h->K, 1), 0.0);
                    rc = run_program_streaming(h, zero.data());
                }
                if (!rc) {
                    const hipError_t e = hipMemcpy(&amp, h->state + h->hf, sizeof(double2), hipMemcpyDeviceToHost);
                    if (e != hipSuccess) rc = fail(h, OVQE_ERR_HIP, hipGetErrorString(e));
                }
            }
            h->prog_set = false;
            if (rc) {
                h->ops.clear();
                h->rots.clear();
                return rc;
            }
            // the Clifford part maps |hf> to a phase times |hf>; the rounding of its quarter turns accumulates with
            // the length of the list (measured 5e-12 after 49 272 gates), hence a tolerance that grows with it
            const double nrm2 = amp.x * amp.x + amp.y * amp.y;
            if (std::fabs(nrm2 - 1.0) > 1e-12 + 1e-15 * (double)tail.size()) return OVQE_OK;  // literal
            const double inv = 1.0 / std::sqrt(nrm2);
            phase = make_double2(amp.x * inv, amp.y * inv);
        }
        drop_tail = true;
    }
    h->prog_set = false;
    h->ops.clear();
    h->rots.clear();
    for (const FrameEmit &e : emitted) push_rotation(h, e.x, e.z, e.coeff, e.phi0, e.pidx);
    if (!drop_tail)
        for (const int64_t g : tail) push_literal_gate(h, opcode[g], b0[g], b1[g], ascale[g], aconst[g], pidx[g]);
    *done = true;
    h->init_amp = phase;  // energies do not depend on it; ovqe_prepare_state reproduces the literal circuit's phase
    return finish_program(h);
}

bool use_small_path(ovqe_handle h, int64_t B) {
    if (h->n_global != 0) return false;
    if (h->opt_force_path == 1) return h->n_local <= 16;
    if (h->opt_force_path == 2) return false;
    if (h->n_local <= h->opt_small_max) return true;
    return h->n_local <= h->opt_small_batch_max && B >= 32;
}

template <bool REAL, bool LDS, int NT, int LBITS>
int launch_small(ovqe_handle h, const SmallArgs &A, int grid, size_t smem) {
    if (int rc = lds_opt_in<&k_small_vqe<REAL, LDS, NT, LBITS>>(h, LDS_WG_MAX)) return rc;
    hipLaunchKernelGGL((k_small_vqe<REAL, LDS, NT, LBITS>), dim3(grid), dim3(NT), smem, h->stream, A,
                       h->cur_theta, (const SmallOp *)h->d_ops.p, (const SmallRot *)h->d_rots.p,
                       (const SmallSeg *)h->d_segs.p, (const ExpGroup *)h->d_egroups.p, (const ExpChunk *)h->d_echunks.p,
                       (const ExpTerm *)h->d_eterms.p, (const FlatItem *)h->d_eflat.p, (const uint16_t *)h->d_stream.p,
                       h->d_workspace.p,
                       h->cur_energies);
    HIPC(h, hipGetLastError());
    return OVQE_OK;
}

// free-index-space expectation tables (sv_small.hpp): one entry per (x-group, pattern of the x-position
// bits) with a non-vanishing coefficient table; the fixed positions are squeezed out of the z masks, the
// sign of parity(x & z), i^ny and the pattern-dependent sign are folded into the coefficients, terms with
// equal outside masks are merged, terms bucketed by the 3 free-index bits above the thread bits
int build_exp_tables(ovqe_handle h, int lbits, bool real) {
    if (h->exp_lbits == lbits && h->exp_real == (int)real && h->exp_ham_version == h->ham.version) return OVQE_OK;
    std::vector<ExpGroup> eg;
    std::vector<ExpTerm> et;
    std::vector<FlatItem> flat;
    const int n = h->n_local;
    // terms the LDS staging area (the idle rotation table) holds
    const int stage_cap = (int)((size_t)h->cs_capacity * sizeof(RotLds) / sizeof(ExpTerm));
    auto squeeze = [](uint64_t z, const int *pos, int np) {  // remove the bit positions pos[] (ascending)
        for (int f = np - 1; f >= 0; --f) {
            const uint64_t low = (1ull << pos[f]) - 1ull;
            z = ((z >> (pos[f] + 1)) << pos[f]) | (z & low);
        }
        return z;
    };
    auto emit = [&](uint32_t x, uint32_t ibits, const int *pos, int np, std::vector<ExpTerm> &list,
                    const std::vector<uint64_t> *zc_index_space) {
        if (list.empty()) return;
        if (zc_index_space && list.size() == 1 && list[0].ci == 0.0 && x != 0 && n <= 16) {
            // single real term: entry-per-lane flat item(s)
            const uint32_t nk = 1u << (n - np);
            const uint32_t nslices = nk >= 64 ? 4 : 1;
            for (uint32_t sl = 0; sl < nslices; ++sl) {
                FlatItem fi;
                fi.x = (uint16_t)x;
                fi.ibits = (uint16_t)ibits;
                fi.zc = (uint16_t)(*zc_index_space)[0];
                fi.slice = (uint16_t)sl;
                fi.count = nk / nslices;
                fi.stride = nslices;
                fi.c = 2.0 * list[0].cr;
                flat.push_back(fi);
            }
            return;
        }
        // a list longer than the staging area becomes consecutive entries with the same pairs: the expectation is linear in the terms
        for (size_t l0 = 0; l0 < list.size(); l0 += (size_t)stage_cap) {
            const size_t l1 = std::min(list.size(), l0 + (size_t)stage_cap);
            ExpGroup out = {};
            out.x = x;
            out.ibits = ibits;
            out.fixmask = 0;
            for (int f = 0; f < np; ++f) out.fixmask |= 1u << pos[f];
            out.t0 = (int32_t)et.size();
            std::vector<ExpTerm> bucket[8];
            for (size_t l = l0; l < l1; ++l) bucket[(list[l].zk >> lbits) & 7].push_back(list[l]);
            int off = 0;
            for (int b = 0; b < 8; ++b) {
                out.off[b] = off;
                for (const ExpTerm &e : bucket[b]) et.push_back(e);
                off += (int)bucket[b].size();
            }
            out.off[8] = off;
            eg.push_back(out);
        }
    };
    for (const HGroup &g : h->ham.groups) {
        const uint64_t x = g.x;
        const int w = __builtin_popcountll(x);
        int pos[64], np = 0;
        for (int b = 0; b < 64; ++b)
            if ((x >> b) & 1) pos[np++] = b;
        // folded coefficients: D uses parity(j & z), j = i ^ x  ->  parity(i & z) ^ parity(x & z)
        std::vector<HTerm> ts;
        for (int t = g.t0; t < g.t1; ++t) {
            HTerm ht = h->ham.terms[t];
            const int ny = __builtin_popcountll(x & ht.z);
            if (real && (ny & 1)) continue;  // imaginary antisymmetric string: zero on a real state
            if (ny & 1) {
                ht.cr = -ht.cr;
                ht.ci = -ht.ci;
            }
            ts.push_back(ht);
        }
        if (ts.empty()) continue;
        if (w == 0 || w > 7 || !h->opt_table_fusion) {
            // dense form: only the pivot is fixed (diag group: nothing fixed)
            const int piv = w ? pos[np - 1] : 0;
            std::vector<ExpTerm> list;
            for (const HTerm &ht : ts) {
                ExpTerm e;
                e.zk = (uint32_t)(w ? squeeze(ht.z, &piv, 1) : ht.z);
                e.pad = 0;
                e.cr = ht.cr;
                e.ci = ht.ci;
                list.push_back(e);
            }
            emit((uint32_t)x, 0, &piv, w ? 1 : 0, list, nullptr);
            continue;
        }
        for (uint32_t e = 0; e < (1u << (w - 1)); ++e) {
            uint64_t ibits = 0;
            for (int f = 0; f < w - 1; ++f)
                if ((e >> f) & 1) ibits |= 1ull << pos[f];
            std::vector<ExpTerm> list;  // merged by outside mask
            std::vector<uint64_t> zcs;  // the outside masks in index space, parallel to list
            for (const HTerm &ht : ts) {
                const uint64_t zc = ht.z & ~x;
                const double sg = (__builtin_popcountll(ibits & ht.z) & 1) ? -1.0 : 1.0;
                const uint32_t zk = (uint32_t)squeeze(zc, pos, np);
                bool found = false;
                for (ExpTerm &q : list)
                    if (q.zk == zk) {
                        q.cr += sg * ht.cr;
                        q.ci += sg * ht.ci;
                        found = true;
                        break;
                    }
                if (!found) {
                    ExpTerm q;
                    q.zk = zk;
                    q.pad = 0;
                    q.cr = sg * ht.cr;
                    q.ci = sg * ht.ci;
                    list.push_back(q);
                    zcs.push_back(zc);
                }
            }
            std::vector<ExpTerm> nz;
            std::vector<uint64_t> nzc;
            for (size_t q = 0; q < list.size(); ++q)
                if (list[q].cr != 0.0 || list[q].ci != 0.0) {  // exact cancellations only
                    nz.push_back(list[q]);
                    nzc.push_back(zcs[q]);
                }
            emit((uint32_t)x, (uint32_t)ibits, pos, np, nz, &nzc);
        }
    }
    // chunks of general groups whose terms fit the LDS staging area (no entry is longer than it: emit)
    std::vector<ExpChunk> chunks;
    {
        ExpChunk cur = {0, 0, 0, 0};
        for (int g = 0; g < (int)eg.size(); ++g) {
            const int gt1 = eg[g].t0 + eg[g].off[8];
            if (gt1 - cur.t0 > stage_cap) {
                if (cur.g1 > cur.g0) chunks.push_back(cur);
                cur = {g, g, eg[g].t0, eg[g].t0};
            }
            cur.g1 = g + 1;
            cur.t1 = gt1;
        }
        if (cur.g1 > cur.g0) chunks.push_back(cur);
    }
    int rc = upload(h, h->d_egroups, eg.data(), eg.size() * sizeof(ExpGroup));
    if (!rc) rc = upload(h, h->d_eterms, et.data(), et.size() * sizeof(ExpTerm));
    if (!rc) rc = upload(h, h->d_echunks, chunks.data(), chunks.size() * sizeof(ExpChunk));
    if (!rc) rc = upload(h, h->d_eflat, flat.data(), flat.size() * sizeof(FlatItem));
    if (rc) return rc;
    h->exp_lbits = lbits;
    h->exp_ham_version = h->ham.version;
    h->exp_real = (int)real;
    h->exp_ngroups = (int)eg.size();
    h->exp_nchunks = (int)chunks.size();
    h->exp_nflat = (int)flat.size();
    return OVQE_OK;
}

// B evaluations with the fused kernel; energies -> host
// host <-> device traffic of a small batch through the mapped buffer: [theta B x K][energies B]
bool mapped_io(ovqe_handle h, int64_t B) {
    // measured: zero-copy wins up to the 64-KiB buffer (H2O: 16 evaluations 63 us against 89 us through copies)
    if ((size_t)B * (size_t)(h->K + 1) > ovqe_sv::IO_DOUBLES || B > 1024) return false;
    if (!h->h_io) {
        if (hipHostMalloc((void **)&h->h_io, ovqe_sv::IO_DOUBLES * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) {
            h->h_io = nullptr;
            (void)hipGetLastError();
            return false;
        }
        if (hipHostGetDevicePointer((void **)&h->d_io, h->h_io, 0) != hipSuccess) {
            (void)hipHostFree(h->h_io);
            h->h_io = nullptr;
            (void)hipGetLastError();
            return false;
        }
    }
    return true;
}

int run_small(ovqe_handle h, int64_t B, const double *theta, double *energies, bool on_device = false) {
    const int n = h->n_local;
    bool real = h->opt_real_mode != 0;
    for (const SmallRot &sr : h->rots) real = real && (sr.ny & 1);
    const size_t amp_bytes = real ? sizeof(double) : sizeof(amp_t);
    const size_t state_bytes = (size_t)h->namps * amp_bytes;
    const bool lds_state = state_bytes <= 128 * 1024;
    const uint64_t npairs = h->namps >> 1;
    const int nt = (!lds_state || npairs >= 1024) ? 1024 : (npairs >= 256 ? 256 : 64);
    const int lbits = nt == 1024 ? 10 : (nt == 256 ? 8 : 6);
    int rc = build_exp_tables(h, lbits, real);
    if (rc) return rc;
    int max_slices = (int)std::max<size_t>(1, std::min<size_t>(512, ((size_t)512 << 20) / state_bytes));
    if (lds_state) max_slices = 1024;
    const int grid = (int)std::min<int64_t>(B, max_slices);
    rc = ensure(h, h->d_workspace, lds_state ? 256 : (size_t)grid * state_bytes);
    if (rc) return rc;
    h->cur_theta = theta;
    h->cur_energies = energies;
    const bool zero_copy = !on_device && mapped_io(h, B);
    const bool poll = zero_copy && B <= 256 && h->opt_poll_result;
    if (zero_copy) {
        if (h->K > 0) std::memcpy(h->h_io, theta, (size_t)B * h->K * sizeof(double));
        if (poll) poll_arm(h->h_io + (size_t)B * h->K, B);
        h->cur_theta = h->d_io;
        h->cur_energies = h->d_io + (size_t)B * h->K;
    } else if (!on_device) {
        rc = ensure(h, h->d_theta, (size_t)B * std::max(1, h->K) * sizeof(double));
        if (rc) return rc;
        rc = ensure(h, h->d_energies, (size_t)B * sizeof(double));
        if (rc) return rc;
        if (h->K > 0)
            HIPC(h, hipMemcpyAsync(h->d_theta.p, theta, (size_t)B * h->K * sizeof(double), hipMemcpyHostToDevice,
                                   h->stream));
        h->cur_theta = (const double *)h->d_theta.p;
        h->cur_energies = (double *)h->d_energies.p;
    }
    SmallArgs A;
    A.n = n;
    A.K = h->K;
    A.nsegs = (int)h->segs.size();
    A.ngroups = h->exp_ngroups;
    A.nchunks = h->exp_nchunks;
    A.nflat = h->exp_nflat;
    A.cs_capacity = h->cs_capacity;
    A.B = B;
    A.constant = h->ham.constant;
    A.hf = h->hf;
    const size_t smem = small_lds(real, lds_state, n, h->cs_capacity).bytes;
    if (!zero_copy) HIPC(h, hipEventRecord(h->ev0, h->stream));
    if (real) {
        if (!lds_state) rc = launch_small<true, false, 1024, 10>(h, A, grid, smem);
        else if (nt == 1024) rc = launch_small<true, true, 1024, 10>(h, A, grid, smem);
        else if (nt == 256) rc = launch_small<true, true, 256, 8>(h, A, grid, smem);
        else rc = launch_small<true, true, 64, 6>(h, A, grid, smem);
    } else {
        if (!lds_state) rc = launch_small<false, false, 1024, 10>(h, A, grid, smem);
        else if (nt == 1024) rc = launch_small<false, true, 1024, 10>(h, A, grid, smem);
        else if (nt == 256) rc = launch_small<false, true, 256, 8>(h, A, grid, smem);
        else rc = launch_small<false, true, 64, 6>(h, A, grid, smem);
    }
    if (rc) return rc;
    h->fused_launch[0] = (real ? 1 : 0) | (lds_state ? 2 : 0) | ((nt == 1024 ? 2 : (nt == 256 ? 1 : 0)) << 2) | (zero_copy ? 16 : 0) |
                         (poll ? 32 : 0) | (on_device ? 64 : 0);
    h->fused_launch[1] = grid;
    h->fused_launch[2] = A.nsegs;
    h->fused_launch[3] = A.nchunks;
    h->fused_launch[4] = A.ngroups;
    h->fused_launch[5] = A.nflat;
    if (zero_copy) {
        if (!poll || !poll_mapped_slots(h->h_io + (size_t)B * h->K, B)) HIPC(h, hipStreamSynchronize(h->stream));
        std::memcpy(energies, h->h_io + (size_t)B * h->K, (size_t)B * sizeof(double));
        h->last_batch_ms = 0.f;  // not timed: no events on the latency path
        return OVQE_OK;
    }
    HIPC(h, hipEventRecord(h->ev1, h->stream));
    if (!on_device)
        HIPC(h, hipMemcpyAsync(energies, h->cur_energies, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    HIPC(h, hipEventElapsedTime(&h->last_batch_ms, h->ev0, h->ev1));
    return OVQE_OK;
}
