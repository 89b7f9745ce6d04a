// abi_unit.inc — C-ABI entry points, unit operations on the resident state (include/ovqe_sv.h).  Included by ovqe_sv.hip inside extern "C".

// ---- unit operations ----------------------------------------------------------------------------
int ovqe_apply_pauli_rotations(ovqe_handle h, int64_t R, const uint64_t *x, const uint64_t *z, const double *phi) try {
    OVQE_ENTER(h);
    if (!h || R < 0 || (R && (!x || !z || !phi))) return OVQE_ERR_INVALID;
    if (R == 0) return OVQE_OK;
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
    // same-x runs, then LDS-tiled multi-run sweeps where consecutive runs fit a tile (sharded registers: the local
    // sweeps between two exchanges arrive here as one list)
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
    // option "real_state": the buffer holds doubles — every string must keep a real state real (odd number of Y, x != 0): the
    // real-amplitude tile sweeps (k_tile_sweep<REAL>: 2^13 amplitudes per 64-KB tile, one more mixing bit per sweep) and pair sweeps
    const bool real = h->opt_real_state != 0;
    if (real) {
        if (h->n_local < 2) return fail(h, OVQE_ERR_INVALID, "real_state needs at least two local qubits");
        for (int64_t r = 0; r < R; ++r)
            if (x[r] == 0 || !(__builtin_popcountll(x[r] & z[r]) & 1))
                return fail(h, OVQE_ERR_INVALID, "real_state: a rotation with an even number of Y (or a diagonal one) makes the amplitudes "
                                                 "complex — clear the option and widen the buffer first");
    }
    TilePlan &tp = h->tp_adhoc;
    if (ops.size() >= 2 && R < (1ll << 30)) {
        rc = build_tile_plan(h, ops, rots, std::vector<uint64_t>(ops.size(), 0), tp, real);
        if (rc) return rc;
    } else {
        tp.plan.assign(ops.size(), 0);
        for (size_t i = 0; i < ops.size(); ++i) tp.plan[i] = -1 - (int32_t)i;
    }
    for (const int32_t step : tp.plan) {
        if (step >= 0) {
            rc = launch_tile_segment(h, tp, tp.tsegs[step], real);
        } else {
            const SmallOp &op = ops[-1 - step];
            if (real) {
                hipLaunchKernelGGL(k_rot_pairs_real, dim3(reduce_blocks(h->namps)), dim3(256), 0, h->stream, (double *)h->state, h->namps >> 1,
                                   op.pivot, op.x, h->base, (const RotParam *)h->d_rp.p + op.first, op.count);
                HIPC(h, hipGetLastError());
                rc = OVQE_OK;
            } else {
                rc = launch_rot_run(h, op.x, (const RotParam *)h->d_rp.p + op.first, op.count);
            }
        }
        if (rc) return rc;
    }
    HIPC(h, hipStreamSynchronize(h->stream));
    h->last_passes = (int64_t)tp.plan.size();               // every step reads and writes the shard once
    h->last_pass_bytes = (int64_t)((real ? 16.0 : 32.0) * (double)h->namps * (double)tp.plan.size());
    return OVQE_OK;
} OVQE_CATCH(h)

int ovqe_apply_pauli_rotation(ovqe_handle h, uint64_t x, uint64_t z, double phi) try {
    OVQE_ENTER(h);
    return ovqe_apply_pauli_rotations(h, 1, &x, &z, &phi);
} OVQE_CATCH(h)

int ovqe_apply_gate(ovqe_handle h, int opcode, int b0, int b1, double angle) try {
    OVQE_ENTER(h);
    if (!h) return OVQE_ERR_INVALID;
    if (b0 < 0 || b0 >= h->n_local) return fail(h, OVQE_ERR_INVALID, "gate bit out of (local) range");
    const uint64_t bit = 1ull << b0;
    int rc;
    switch (opcode) {
    case OVQE_GATE_X: rc = launch_gate(h, 0, b0, 0); break;
    case OVQE_GATE_H: rc = launch_gate(h, 1, b0, 0); break;
    case OVQE_GATE_RX: return ovqe_apply_pauli_rotation(h, bit, 0, 0.5 * angle);
    case OVQE_GATE_RY: return ovqe_apply_pauli_rotation(h, bit, bit, 0.5 * angle);
    case OVQE_GATE_RZ: return ovqe_apply_pauli_rotation(h, 0, bit, 0.5 * angle);
    case OVQE_GATE_CNOT:
        if (b1 < 0 || b1 >= h->n_local || b1 == b0) return fail(h, OVQE_ERR_INVALID, "CNOT target bit invalid");
        rc = launch_gate(h, 2, b0, b1);
        break;
    default: return fail(h, OVQE_ERR_INVALID, "unknown gate opcode");
    }
    if (rc) return rc;
    HIPC(h, hipStreamSynchronize(h->stream));
    return OVQE_OK;
} OVQE_CATCH(h)

int ovqe_bilinear(ovqe_handle h, const void *bra_dev, const void *ket_dev, int64_t T, const uint64_t *x,
                  const uint64_t *z, const double *coeff_re, const double *coeff_im, double *out_re_im) try {
    OVQE_ENTER(h);
    if (!h || T < 0 || !out_re_im || (T && (!x || !z || !coeff_re))) return OVQE_ERR_INVALID;
    bool real_coeffs = true;  // real coefficients: every term is Hermitian -> pair-trick kernels when bra == ket
    if (coeff_im)
        for (int64_t t = 0; t < T; ++t) real_coeffs = real_coeffs && coeff_im[t] == 0.0;
    if (!bra_dev && !ket_dev && real_coeffs && T > 0) {
        // <state|H|state> of a Hermitian sum: kept (with its tile cover) until a different sum arrives — a sharded
        // register evaluates the same local term list once per energy
        HamDev &H = h->ham_adhoc;
        const bool same = H.set && (int64_t)h->adhoc_x.size() == T &&
                          std::equal(x, x + T, h->adhoc_x.begin()) && std::equal(z, z + T, h->adhoc_z.begin()) &&
                          std::equal(coeff_re, coeff_re + T, h->adhoc_c.begin());
        if (!same) {
            H.set = false;
            int rc = build_groups(h, T, x, z, coeff_re, nullptr, false, H.groups, H.terms);
            if (rc) return rc;
            rc = upload(h, H.d_groups, H.groups.data(), H.groups.size() * sizeof(HGroup));
            if (!rc) rc = upload(h, H.d_terms, H.terms.data(), H.terms.size() * sizeof(HTerm));
            if (rc) return rc;
            h->adhoc_x.assign(x, x + T);
            h->adhoc_z.assign(z, z + T);
            h->adhoc_c.assign(coeff_re, coeff_re + T);
            H.tile_bits = -1;
            H.set = true;
        }
        double2 res = make_double2(0.0, 0.0);
        bool tiled = false;
        int rc = run_expectation_tiled(h, H, &res, &tiled);
        if (!rc && !tiled)
            rc = run_bilinear(h, h->state, h->state, H.groups, (const HGroup *)H.d_groups.p, (const HTerm *)H.d_terms.p,
                              &res, true);
        out_re_im[0] = res.x;
        out_re_im[1] = res.y;
        return rc;
    }
    std::vector<HGroup> groups;
    std::vector<HTerm> terms;
    int rc = build_groups(h, T, x, z, coeff_re, coeff_im, /*allow_global_x=*/ket_dev != nullptr, groups, terms);
    if (rc) return rc;
    // (the handle's pool buffers carry the term list: a sharded <H> makes tens of thousands of these calls, one per partner chunk)
    rc = upload(h, h->d_pg_xs, groups.data(), std::max<size_t>(groups.size(), 1) * sizeof(HGroup));
    if (!rc) rc = upload(h, h->d_pg_terms, terms.data(), std::max<size_t>(terms.size(), 1) * sizeof(HTerm));
    h->pg_valid = false;  // the pool buffers were borrowed
    double2 res = make_double2(0.0, 0.0);
    if (!rc)
        rc = run_bilinear(h, bra_dev ? (const amp_t *)bra_dev : h->state, ket_dev ? (const amp_t *)ket_dev : h->state,
                          groups, (const HGroup *)h->d_pg_xs.p, (const HTerm *)h->d_pg_terms.p, &res, false);
    out_re_im[0] = res.x;
    out_re_im[1] = res.y;
    return rc;
} OVQE_CATCH(h)

int ovqe_apply_pauli_sum(ovqe_handle h, const void *ket_dev, void *out_dev, int64_t T, const uint64_t *x, const uint64_t *z,
                         const double *coeff_re, const double *coeff_im, int accumulate) try {
    OVQE_ENTER(h);
    if (!h || !out_dev || T < 0 || (T && (!x || !z || !coeff_re))) return OVQE_ERR_INVALID;
    const amp_t *ket = ket_dev ? (const amp_t *)ket_dev : h->state;
    if ((const void *)ket == out_dev) return fail(h, OVQE_ERR_INVALID, "ovqe_apply_pauli_sum: out must differ from the ket");
    if (T == 0) {   // the empty sum: out = 0, or out unchanged when accumulating
        if (!accumulate) HIPC(h, hipMemsetAsync(out_dev, 0, (size_t)h->namps * sizeof(amp_t), h->stream));
        HIPC(h, hipStreamSynchronize(h->stream));
        return OVQE_OK;
    }
    std::vector<HGroup> groups;
    std::vector<HTerm> terms;
    int rc = build_groups(h, T, x, z, coeff_re, coeff_im, /*allow_global_x=*/ket_dev != nullptr, groups, terms);
    if (rc) return rc;
    rc = upload(h, h->d_pg_xs, groups.data(), std::max<size_t>(groups.size(), 1) * sizeof(HGroup));
    if (!rc) rc = upload(h, h->d_pg_terms, terms.data(), std::max<size_t>(terms.size(), 1) * sizeof(HTerm));
    if (rc) return rc;
    h->pg_valid = false;  // the pool buffers were borrowed
    hipLaunchKernelGGL(k_apply_terms, dim3(reduce_blocks(h->namps)), dim3(256), 0, h->stream, (amp_t *)out_dev, ket, h->namps,
                       (const HGroup *)h->d_pg_xs.p, (int)groups.size(), (const HTerm *)h->d_pg_terms.p, accumulate);
    HIPC(h, hipGetLastError());
    HIPC(h, hipStreamSynchronize(h->stream));
    return OVQE_OK;
} OVQE_CATCH(h)

int ovqe_bilinear_batch(ovqe_handle h, const void *bra_dev, const void *ket_dev, int64_t n_ops, const int64_t *offsets,
                        const uint64_t *x, const uint64_t *z, const double *coeff_re, const double *coeff_im,
                        double *out_re_im) try {
    OVQE_ENTER(h);
    if (!h || n_ops < 0 || !offsets || (n_ops && !out_re_im)) return OVQE_ERR_INVALID;
    if (n_ops == 0) return OVQE_OK;
    const int64_t T = offsets[n_ops];
    if (T < 0 || (T && (!x || !z || !coeff_re))) return OVQE_ERR_INVALID;
    if (T == 0) {   // operators without terms: every bilinear form is 0
        std::fill(out_re_im, out_re_im + 2 * n_ops, 0.0);
        return OVQE_OK;
    }
    const uint64_t lmask = local_mask(h);
    std::vector<HTerm> terms(T);
    std::vector<uint64_t> xs(T);
    uint64_t xg = 0;
    for (int64_t t = 0; t < T; ++t) {
        if (t == 0) xg = x[t] & ~lmask;
        if ((x[t] & ~lmask) != xg) return fail(h, OVQE_ERR_INVALID, "ovqe_bilinear_batch: one global x part per call");
        HTerm ht;
        ht.z = z[t];
        fold_iny(coeff_re[t], coeff_im ? coeff_im[t] : 0.0, __builtin_popcountll(x[t] & z[t]), ht.cr, ht.ci);
        terms[t] = ht;
        xs[t] = x[t] & lmask;
    }
    if (xg && !ket_dev) return fail(h, OVQE_ERR_INVALID, "x mask touches global (rank) bits: pass the partner's shard as ket");
    for (int64_t k = 0; k < n_ops; ++k)
        if (offsets[k] > offsets[k + 1] || offsets[k] < 0) return fail(h, OVQE_ERR_INVALID, "offsets not monotone");
    h->pg_valid = false;
    int rc = upload(h, h->d_pg_off, offsets, (n_ops + 1) * sizeof(int64_t));
    if (!rc) rc = upload(h, h->d_pg_xs, xs.data(), std::max<int64_t>(T, 1) * sizeof(uint64_t));
    if (!rc) rc = upload(h, h->d_pg_terms, terms.data(), std::max<int64_t>(T, 1) * sizeof(HTerm));
    const int nchunks = h->n_local <= 22 ? 1 : (int)(h->namps >> 16);
    const int64_t ops_per_launch = 32768;
    if (!rc) rc = ensure(h, h->d_pg_out, n_ops * sizeof(double2));
    if (!rc && nchunks > 1)
        rc = ensure(h, h->d_pg_part, (size_t)std::min<int64_t>(n_ops, ops_per_launch) * nchunks * sizeof(double2));
    if (rc) return rc;
    const amp_t *bra = bra_dev ? (const amp_t *)bra_dev : h->state, *ket = ket_dev ? (const amp_t *)ket_dev : h->state;
    const uint64_t ket_base = (h->base ^ xg) & ~lmask;
    for (int64_t op0 = 0; op0 < n_ops; op0 += ops_per_launch) {
        const int64_t cnt = std::min<int64_t>(ops_per_launch, n_ops - op0);
        double2 *out = (double2 *)h->d_pg_out.p + op0;
        double2 *part = nchunks > 1 ? (double2 *)h->d_pg_part.p : out;
        hipLaunchKernelGGL(k_pool_grad, dim3((unsigned)nchunks, (unsigned)cnt), dim3(256), 0, h->stream, bra, ket, h->namps,
                           ket_base, (const int64_t *)h->d_pg_off.p, (const uint64_t *)h->d_pg_xs.p,
                           (const HTerm *)h->d_pg_terms.p, op0, part);
        if (nchunks > 1)
            hipLaunchKernelGGL(k_reduce_rows2, dim3((unsigned)cnt), dim3(256), 0, h->stream, (const double2 *)part, nchunks, out);
    }
    HIPC(h, hipGetLastError());
    HIPC(h, hipMemcpyAsync(out_re_im, h->d_pg_out.p, n_ops * sizeof(double2), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    return OVQE_OK;
} OVQE_CATCH(h)

int ovqe_expectation(ovqe_handle h, int64_t T, const uint64_t *x, const uint64_t *z, const double *coeff,
                     double constant, double *out) try {
    OVQE_ENTER(h);
    if (!out) return OVQE_ERR_INVALID;
    double res[2] = {0.0, 0.0};
    int rc = ovqe_bilinear(h, nullptr, nullptr, T, x, z, coeff, nullptr, res);
    if (rc) return rc;
    *out = res[0] + constant;
    return OVQE_OK;
} OVQE_CATCH(h)

// ---- k-bit shard exchange: pack / unpack of one block (csrc/sv_kernels.hpp, k_shard_copy).  Both only enqueue on the handle's stream.
extern "C++" {
namespace {
template <bool PACK>
int shard_copy(ovqe_handle h, uint64_t mask, uint64_t block, int64_t first, int64_t count, void *buf, int real_parts_only) {
    const char *who = PACK ? "ovqe_shard_pack" : "ovqe_shard_unpack";
    if (!h) return OVQE_ERR_INVALID;
    if (!buf) return fail(h, OVQE_ERR_INVALID, std::string(who) + ": null buffer");
    const int k = __builtin_popcountll(mask);
    if (mask == 0 || (mask & ~local_mask(h)) || k > 6)
        return fail(h, OVQE_ERR_INVALID, std::string(who) + ": the mask names 1 to 6 local bits of this shard");
    if (block >> k) return fail(h, OVQE_ERR_INVALID, std::string(who) + ": block value beyond the exchanged bits");
    const uint64_t bsize = h->namps >> k;
    if (first < 0 || count < 0 || (uint64_t)first > bsize || (uint64_t)count > bsize - (uint64_t)first)
        return fail(h, OVQE_ERR_INVALID, std::string(who) + ": range past the block");
    const bool stored_real = h->opt_real_state != 0;
    if (stored_real && real_parts_only) real_parts_only = 0;   // (8-byte amplitudes travel as they are)
    if ((uintptr_t)buf & ((stored_real || real_parts_only) ? 7u : 15u))
        return fail(h, OVQE_ERR_INVALID, std::string(who) + ": buffer not aligned to its elements");
    if (count == 0) return OVQE_OK;
    // 16-byte units of two 8-byte elements where the shard side keeps them adjacent (bit 0 not exchanged, even range, aligned buffer)
    const bool pair = (stored_real || real_parts_only) && !(mask & 1) && !(first & 1) && !(count & 1) && !((uintptr_t)buf & 15u) &&
                      h->n_local >= 2;
    const int sh = pair ? 1 : 0;
    uint64_t m = mask >> sh, fixed = 0;
    BitRuns R = {};
    for (int bit = 0, i = 0; bit < 64 - sh; ++bit)   // deposit(block, mask), in units
        if ((m >> bit) & 1) fixed |= ((block >> i++) & 1ull) << bit;
    R.fixed = fixed;
    while (m) {
        const int pos = __builtin_ctzll(m);
        int len = 0;
        while ((m >> (pos + len)) & 1) ++len;
        R.pos[R.n] = (uint8_t)pos;
        R.len[R.n] = (uint8_t)len;
        ++R.n;
        m &= ~(((1ull << len) - 1ull) << pos);
    }
    const uint64_t f = (uint64_t)first >> sh, c = (uint64_t)count >> sh;
    if (real_parts_only) {
        const dim3 grid((unsigned)std::min<uint64_t>(1u << 30, (c + 511) / 512));   // (one trip per lane: see k_shard_copy)
        if (pair) hipLaunchKernelGGL((k_shard_copy_re<true, PACK>), grid, dim3(256), 0, h->stream, h->state, (double *)buf, f, c, R);
        else hipLaunchKernelGGL((k_shard_copy_re<false, PACK>), grid, dim3(256), 0, h->stream, h->state, (double *)buf, f, c, R);
    } else {
        const dim3 grid((unsigned)std::min<uint64_t>(1u << 30, (c + 1023) / 1024));
        if (stored_real && !pair)
            hipLaunchKernelGGL((k_shard_copy<double, PACK>), grid, dim3(256), 0, h->stream, (double *)h->state, (double *)buf, f, c, R);
        else
            hipLaunchKernelGGL((k_shard_copy<double2, PACK>), grid, dim3(256), 0, h->stream, (double2 *)h->state, (double2 *)buf, f, c, R);
    }
    HIPC(h, hipGetLastError());
    return OVQE_OK;
}
}  // namespace
}  // extern "C++"

int ovqe_shard_pack(ovqe_handle h, uint64_t local_bit_mask, uint64_t block, int64_t first, int64_t count, void *dst,
                    int real_parts_only) try {
    OVQE_ENTER(h);
    return shard_copy<true>(h, local_bit_mask, block, first, count, dst, real_parts_only);
} OVQE_CATCH(h)

int ovqe_shard_unpack(ovqe_handle h, uint64_t local_bit_mask, uint64_t block, int64_t first, int64_t count, const void *src,
                      int real_parts_only) try {
    OVQE_ENTER(h);
    return shard_copy<false>(h, local_bit_mask, block, first, count, const_cast<void *>(src), real_parts_only);
} OVQE_CATCH(h)
