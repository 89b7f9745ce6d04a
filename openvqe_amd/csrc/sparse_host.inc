// sparse_host.inc — the support-compacted path (states whose program reaches few basis states): table build and launches
// (kernels: sv_sparse.hpp).  Included by ovqe_sv.hip inside its anonymous namespace.

// Instances of the workgroup geometry of the rows form (k_sparse_vqe_rows_shared<NW, RPT, EPR, SSTRIDE>), smaller first.  An instance
// holds a program when its entries are at most 64 NW x EPT (the capacity criterion its name carries), its state fits the stride, its
// LDS fits half a CU (launch_rows_shared) AND the entries pack into 64 NW x RPT owner pieces of EPR slots (sparse_pack.hpp).  The
// shapes RPT x EPR are the measured ones of profiles/owner_rows/README.md.  te: the pipelined item loop (sv_sparse.hpp) keeps the table
// records of 32 te distinct angles in registers (profiles/pipelined_rows/README.md).  Both instances: no scratch.  H2O 252 VGPRs, two
// waves per SIMD; LiH 164, THREE waves per SIMD (three workgroups per CU; four with the plain loop, which was slower at every batch size).
// Both are four registers under the next step (256, 168): the contraction holds one slot group in flight (profiles/contraction_ahead).
struct SharedInstance { int nw, ept, sstride, rpt, epr, te; };
constexpr SharedInstance SHARED_13 = {4, 13, 2568, 1, 17, 3};   // LiH: 225 states, 3243 entries: 18 LDS reads per thread and state
constexpr SharedInstance SHARED_37 = {4, 37, 4104, 4, 10, 5};   // H2O: 441 states, 9443 entries: 44
constexpr SharedInstance SHARED_INSTANCES[2] = {SHARED_13, SHARED_37};

// ---- support-compacted path (sv_sparse.hpp) -------------------------------------------------------------------
// Propagate the reachable support of |hf> through the OP_TAB ops and restate program and Hamiltonian on compact
// indices.  Returns with h->sp_valid = false when the structure is absent (then the dense kernels run).
int build_sparse_program(ovqe_handle h) {
    h->sp_tried = true;
    h->sp_valid = false;
    if (!h->opt_sparse || !h->opt_table_fusion || !h->opt_real_mode || h->n_global != 0 || h->n_local > 40) return OVQE_OK;
    if (!h->prog_set || !h->ham.set || h->K <= 0) return OVQE_OK;
    for (const SmallRot &sr : h->rots)
        if (!(sr.ny & 1)) return OVQE_OK;  // real mode only
    for (const SmallOp &op : h->sops)
        if (op.kind != OP_TAB || op.count > 127) return OVQE_OK;
    const int MAXM = 4096;
    std::unordered_map<uint64_t, int> id;
    std::vector<uint64_t> S;
    auto get = [&](uint64_t a) {
        auto it = id.find(a);
        if (it != id.end()) return it->second;
        const int k = (int)S.size();
        id.emplace(a, k);
        S.push_back(a);
        return k;
    };
    get(h->hf);
    std::vector<SpOp> ops;
    std::vector<uint32_t> pairs;
    for (const SmallOp &op : h->sops) {
        const uint64_t x = op.x, pbit = 1ull << (63 - __builtin_clzll(x));
        SpOp so;
        so.first = (int32_t)pairs.size();
        so.tab0 = op.first;
        so.pad = 0;
        const size_t s0 = S.size();
        std::unordered_set<uint64_t> seen;
        for (size_t k = 0; k < s0; ++k) {
            const uint64_t a = S[k];
            const uint64_t i0 = (a & pbit) ? (a ^ x) : a;
            if (!seen.insert(i0).second) continue;
            for (int p = 0; p < op.count; ++p) {
                if ((i0 & x) != h->srots[op.first + p].z) continue;
                const int ci = get(i0), cj = get(i0 ^ x);
                if ((int)S.size() > MAXM) return OVQE_OK;
                const uint32_t sgn = (__builtin_popcountll(i0 & (uint64_t)op.zc) & 1) ? 1u : 0u;
                pairs.push_back((uint32_t)ci | ((uint32_t)cj << 12) | (sgn << 24) | ((uint32_t)p << 25));
                break;
            }
        }
        so.npairs = (int32_t)pairs.size() - so.first;
        if (so.npairs > 0) ops.push_back(so);
    }
    const int m = (int)S.size();
    // Hamiltonian restricted to the support (real mode: even-ny terms; pair counted once -> factor 2): the one rule of sv_constrain_host.hpp
    std::vector<SpEntry> entries;
    if (!constrain::restrict_to_support(h->ham.groups, h->ham.terms, S.data(), m, [&](uint64_t a) {
            auto it = id.find(a);
            return it == id.end() ? -1 : it->second;
        }, constrain::ENTRY_CAP, &entries))
        return OVQE_OK;
    // whether these entries ARE H on the support: what the loop above dropped — partners outside the support, terms with an odd number
    // of Y — is exact for <H> on a real state and wrong for <H^2> (ovqe_spread_gradient_batch takes its compact path only with neither)
    const spread::Exactness exact = spread::exactness(h->ham.groups, h->ham.terms, S, [&](uint64_t a) { return id.find(a) != id.end(); });
    // ---- compact numbering, lanes and orientation against LDS bank conflicts in the circuit: the planner (sparse_plan.hpp) -----------
    // The lanes of an evaluation rotate the (up to 32) pairs of an op with ONE ds_read_b64 per member and one ds_write_b64 each; which
    // banks they meet on is the host's to choose.  The entries of the restricted Hamiltonian follow the numbering.
    SparsePlan plan;
    {
        std::vector<PlanOp> pops;
        for (const SpOp &so : ops) pops.push_back({so.first, so.npairs});
        plan_sparse_program(m, pops, pairs, h->opt_sparse_renumber != 0, &plan);
    }
    pairs.swap(plan.pairs);
    const int mp = plan.mp, hf_slot = plan.slot[0];
    h->sp_conflicts_before = plan.conflicts_discovery;
    h->sp_conflicts_after = plan.conflicts;
    for (SpEntry &e : entries) e.ij = (uint32_t)plan.slot[e.ij & 0xfffu] | ((uint32_t)plan.slot[(e.ij >> 12) & 0xfffu] << 12);
    arrange_entries(entries);   // (the entry stream of the per-wave kernels)
    // rows of 32 padded 64-bit words for the throughput kernel (k_sparse_vqe_rows): only when every byte offset fits 16 bits
    std::vector<uint64_t> rows;
    h->sp_nrows4 = 0;
    const int ntab_all = (int)h->srots.size();
    // ... with ONE cos/sin entry per distinct angle: table entries of one parameter with coefficients +-c (the active patterns of
    // a JW excitation) share cos and differ in the sign of sin, which moves into the word's sign bit — fewer sincos per evaluation
    // and a smaller table per evaluation in LDS (more waves per CU)
    std::vector<SmallRot> prim;
    std::vector<int> prim_of((size_t)ntab_all, -1);
    std::vector<uint8_t> prim_neg((size_t)ntab_all, 0);
    {
        std::unordered_map<uint64_t, std::vector<int>> by_param;
        for (int e = 0; e < ntab_all; ++e) {
            const SmallRot &sr = h->srots[e];
            std::vector<int> &cand = by_param[(uint64_t)(uint32_t)sr.pidx];
            for (int p : cand)
                if (std::fabs(prim[p].coeff) == std::fabs(sr.coeff) && prim[p].phi0 == 0.0 && sr.phi0 == 0.0) {
                    prim_of[e] = p;
                    prim_neg[e] = (prim[p].coeff < 0) != (sr.coeff < 0);
                    break;
                }
            if (prim_of[e] < 0) {
                prim_of[e] = (int)prim.size();
                cand.push_back((int)prim.size());
                prim.push_back(sr);
            }
        }
    }
    const int nprim = (int)prim.size();
    h->sp_nprim = 0;
    if (h->opt_sparse_rows && (size_t)(mp + 64) * 8 < 65536 && (size_t)(nprim + 1) * 16 < 65536) {
        auto pad_word = [&](int lane) {
            return (uint64_t)((uint32_t)(mp + lane) * 8u) | ((uint64_t)((uint32_t)(mp + 32 + lane) * 8u) << 16) |
                   ((uint64_t)((uint32_t)nprim * 16u) << 32);
        };
        size_t at = 0;   // the planner's rows: those of an op in a block, ops in order
        for (const SpOp &so : ops)
            for (int c0 = 0; c0 < so.npairs; c0 += 32)
                for (int lane = 0; lane < 32; ++lane) {
                    const RowLane &rl = plan.rows[at++];
                    const uint64_t slots = (uint64_t)(rl.si * 8u) | ((uint64_t)(rl.sj * 8u) << 16);
                    if (rl.pair < 0) {
                        rows.push_back(slots | ((uint64_t)((uint32_t)nprim * 16u) << 32));
                        continue;
                    }
                    const uint32_t pw = pairs[(size_t)rl.pair], ent = (uint32_t)so.tab0 + (pw >> 25);
                    const bool neg = ((pw >> 24) & 1u) != (uint32_t)prim_neg[ent];   // (the word's sign is the orientation's)
                    rows.push_back(slots | ((uint64_t)((uint32_t)prim_of[ent] * 16u) << 32) | (neg ? (1ull << 63) : 0ull));
                }
        const int nrows = (int)(rows.size() / 32);
        const int nrows4 = (nrows + 3) & ~3;
        for (int r = nrows; r < nrows4 + 4; ++r)             // padding to a multiple of four + the four rows fetched ahead
            for (int lane = 0; lane < 32; ++lane) rows.push_back(pad_word(lane));
        h->sp_nrows4 = nrows4;
        h->sp_nprim = nprim;
    }
    // ... and rows of 64 for the latency kernel (one evaluation per workgroup, the circuit on its first wave; byte offsets
    // slot * 8, spare slots mp .. mp + 127)
    std::vector<uint64_t> rows64;
    h->sp_nrows8 = 0;
    if (h->opt_sparse_rows && (size_t)(mp + 128) * 8 < 65536 && (size_t)(nprim + 1) * 16 < 65536) {
        auto pad_word = [&](int lane) {
            return (uint64_t)((uint32_t)(mp + lane) * 8u) | ((uint64_t)((uint32_t)(mp + 64 + lane) * 8u) << 16) |
                   ((uint64_t)((uint32_t)nprim * 16u) << 32);
        };
        // a row of 64 is two of the planner's rows of 32 side by side (a read is served per 32 lanes, a write per 16: the banks they
        // were chosen on hold); the pads of the upper half move to the upper 32 spare slots of each range
        size_t at = 0;
        for (const SpOp &so : ops) {
            const int nch = (so.npairs + 31) / 32;
            for (int c = 0; c < nch; c += 2) {
                const int halves = std::min(2, nch - c);
                // padded lanes rotate their (zero) spare slots by the cos/sin entry of the row's FIRST pair: rows of one entry stay
                // uniform for the gradient kernel's wave sums
                uint32_t ent0 = (uint32_t)nprim;
                for (int l = 0; l < 32 * halves; ++l)
                    if (plan.rows[at + l].pair >= 0) {
                        ent0 = (uint32_t)prim_of[(uint32_t)so.tab0 + (pairs[(size_t)plan.rows[at + l].pair] >> 25)];
                        break;
                    }
                for (int hh = 0; hh < 2; ++hh)
                    for (int l = 0; l < 32; ++l) {
                        if (hh >= halves) {
                            rows64.push_back((pad_word(32 + l) & 0xffffffffull) | ((uint64_t)(ent0 * 16u) << 32));
                            continue;
                        }
                        const RowLane &rl = plan.rows[at + 32 * hh + l];
                        if (rl.pair < 0) {
                            const uint32_t si = rl.si + 32u * hh, sj = rl.sj + 32u + 32u * hh;
                            rows64.push_back((uint64_t)(si * 8u) | ((uint64_t)(sj * 8u) << 16) | ((uint64_t)(ent0 * 16u) << 32));
                            continue;
                        }
                        const uint32_t pw = pairs[(size_t)rl.pair], ent = (uint32_t)so.tab0 + (pw >> 25);
                        const bool neg = ((pw >> 24) & 1u) != (uint32_t)prim_neg[ent];
                        rows64.push_back((uint64_t)(rl.si * 8u) | ((uint64_t)(rl.sj * 8u) << 16) |
                                         ((uint64_t)((uint32_t)prim_of[ent] * 16u) << 32) | (neg ? (1ull << 63) : 0ull));
                    }
                at += (size_t)32 * halves;
            }
        }
        const int nrows = (int)(rows64.size() / 64);
        const int nrows8 = (nrows + 7) & ~7;
        for (int r = nrows; r < nrows8 + 8; ++r)
            for (int lane = 0; lane < 64; ++lane) rows64.push_back(pad_word(lane));
        h->sp_nrows8 = nrows8;
    }
    // owner pieces of the restricted Hamiltonian for the first instance of the workgroup geometry that holds the program
    h->sp_pack_inst = -1;
    h->sp_h_pieces = h->sp_h_rpt = h->sp_h_epr = 0;
    // modelled LDS array cycles per evaluation (ovqe_program_info [33..37])
    h->sp_cycles[0] = plan.cycles.reads;
    h->sp_cycles[1] = plan.cycles.writes;
    h->sp_cycles[2] = 0;
    h->sp_cycles[3] = plan.cycles_discovery.reads;
    h->sp_cycles[4] = plan.cycles_discovery.writes;
    std::vector<unsigned char> hpack;
    if (h->sp_nrows4 && !entries.empty() && h->opt_sparse_pack) {
        std::vector<uint32_t> ei(entries.size()), ej(entries.size());
        std::vector<double> ec(entries.size());
        for (size_t e = 0; e < entries.size(); ++e) {
            ei[e] = entries[e].ij & 0xfffu;
            ej[e] = (entries[e].ij >> 12) & 0xfffu;
            ec[e] = entries[e].c;
        }
        const size_t state_bytes = (size_t)((mp + 64 + 1) & ~1) * sizeof(double);   // run_sparse: the rows form's state + spare slots
        for (int k = 0; k < 2 && h->sp_pack_inst < 0; ++k) {
            const SharedInstance &I = SHARED_INSTANCES[k];
            const int nt = 64 * I.nw;
            if (entries.size() > (size_t)nt * I.ept || state_bytes > (size_t)I.sstride) continue;
            OwnerPack P;
            if (!pack_owner_pieces(ei, ej, ec, mp, nt, I.rpt, I.epr, &P)) continue;
            hpack.resize(P.c.size() * sizeof(double) + (P.oj.size() + P.oi.size()) * sizeof(uint16_t));
            std::memcpy(hpack.data(), P.c.data(), P.c.size() * sizeof(double));
            std::memcpy(hpack.data() + P.c.size() * sizeof(double), P.oj.data(), P.oj.size() * sizeof(uint16_t));
            std::memcpy(hpack.data() + P.c.size() * sizeof(double) + P.oj.size() * sizeof(uint16_t), P.oi.data(), P.oi.size() * sizeof(uint16_t));
            h->sp_pack_inst = k;
            h->sp_h_pieces = P.pieces;
            h->sp_h_rpt = I.rpt;
            h->sp_h_epr = I.epr;
            const PackCycles pc = pack_cycles(P);
            h->sp_cycles[2] = pc.slot_reads + pc.owner_reads;
        }
    }
    int rc = upload(h, h->d_sp_ops, ops.data(), ops.size() * sizeof(SpOp));
    if (!rc && h->sp_pack_inst >= 0) rc = upload(h, h->d_sp_hpack, hpack.data(), hpack.size());
    if (!rc && h->sp_nrows4) rc = upload(h, h->d_sp_rows, rows.data(), rows.size() * sizeof(uint64_t));
    if (!rc && (h->sp_nrows4 || h->sp_nrows8)) rc = upload(h, h->d_sp_prim, prim.data(), prim.size() * sizeof(SmallRot));
    if (!rc && h->sp_nrows8) rc = upload(h, h->d_sp_rows64, rows64.data(), rows64.size() * sizeof(uint64_t));
    if (!rc) rc = upload(h, h->d_sp_pairs, pairs.data(), pairs.size() * sizeof(uint32_t));
    if (!rc) rc = upload(h, h->d_sp_entries, entries.data(), entries.size() * sizeof(SpEntry));
    if (!rc) {   // the basis index behind every slot (k_deflate_gather restricts the deflation vectors to the support with it)
        std::vector<uint64_t> &basis = h->sp_basis;   // (the host copy: the observables of constrain_host.inc are restricted with it)
        basis.assign(((size_t)mp + 1) & ~(size_t)1, ~0ull);
        for (int k = 0; k < m; ++k) basis[(size_t)plan.slot[k]] = S[k];
        rc = upload(h, h->d_sp_basis, basis.data(), basis.size() * sizeof(uint64_t));
    }
    if (rc) return rc;
    ++h->sp_build;
    h->sp_exact = exact;
    h->sp_m = m;
    h->sp_mp = mp;
    h->sp_hf = hf_slot;
    h->sp_nops = (int)ops.size();
    h->sp_nent = (int)entries.size();
    h->sp_npairs = (int64_t)pairs.size();
    h->sp_valid = true;
    return OVQE_OK;
}

template <int SPW, bool STAGE = false>
int launch_sparse(ovqe_handle h, const SparseArgs &A, int grid, size_t smem) {
    if (int rc = lds_opt_in<&k_sparse_vqe<SPW, STAGE>>(h, LDS_WG_MAX)) return rc;
    hipLaunchKernelGGL((k_sparse_vqe<SPW, STAGE>), dim3(grid), dim3(64), smem, h->stream, A, h->cur_theta,
                       (const SmallRot *)h->d_rots.p, (const SpOp *)h->d_sp_ops.p, (const uint32_t *)h->d_sp_pairs.p,
                       (const SpEntry *)h->d_sp_entries.p, h->cur_energies);
    HIPC(h, hipGetLastError());
    return OVQE_OK;
}

// which forms served a handle since its program was set (ovqe_last_support which = 7; the tests name the geometry behind each)
enum : uint32_t {
    SPF_WG = 1u << 0,            // k_sparse_vqe_wg: one evaluation per workgroup (B <= 256)
    SPF_STAGED1 = 1u << 1,       // k_sparse_vqe<1, true>: op table and pair words staged in LDS (B <= 1024)
    SPF_PLAIN1 = 1u << 2,        // k_sparse_vqe<1, false>
    SPF_ROWS2 = 1u << 3,         // k_sparse_vqe_rows<2> / k_sparse_vqe_rows_shared: the throughput form (B >= 2048), geometry in SPG_*
    SPF_PLAIN2 = 1u << 4,        // k_sparse_vqe<2, false> (no row tables)
    SPF_PLAIN4 = 1u << 5,        // k_sparse_vqe<4, false> ("sparse_spw" = 4)
    SPF_GRAD_WG = 1u << 6,       // k_sparse_grad_wg
    SPF_GRAD_STAGED = 1u << 7,   // k_sparse_grad<true>
    SPF_GRAD_PLAIN = 1u << 8,    // k_sparse_grad<false>
    SPF_DECLINED = 1u << 9,      // a call wanted the compact path and no form of it fits: the other paths served it
    // launch geometry of SPF_ROWS2 (bits the form names do not reach: Statevector.sparse_geometries())
    SPG_PER_WAVE = 1u << 10,     // k_sparse_vqe_rows<2>: one wave per pair of evaluations, the Hamiltonian's entries streamed from L2
    // ... the instances of k_sparse_vqe_rows_shared (entries in registers as owner pieces).  The names ("shared_e37_s4104",
    // "shared_e13_s2568" in backend.py) identify the INSTANCE — its capacity criterion, 37 / 13 entries per thread, and its stride —
    // not the slot layout of the pieces (SHARED_37 / SHARED_13 above)
    SPG_SHARED_37 = 1u << 11,    // k_sparse_vqe_rows_shared<4, 4, 10, 4104, ...>  (H2O: 441 states, 9443 entries)
    SPG_SHARED_13 = 1u << 12,    // k_sparse_vqe_rows_shared<4, 1, 17, 2568, ...>  (LiH: 225 states)
};

// the workgroup geometry of the rows form: batches from SHARED_MIN_B on — measured (tools/exp_shared_sweep.py, profiles/shared_rows): it
// wins beyond the spread at every batch size the rows form takes, 2048 included (H2O: 35.6 against 40.3 us)
constexpr int64_t SHARED_MIN_B = 2048;

template <int NW, int RPT, int EPR, int SSTRIDE, int TE, int DBG>
int launch_rows_shared_dbg(ovqe_handle h, const SparseArgs &R, size_t smem) {
    constexpr int NS = 2 * NW;
    // workgroups one CU holds at once at this much LDS, cached per device: both in ONE word (smem << 8 | per_cu; smem <= 80 KiB,
    // per_cu <= 32), so that two threads with a handle each never see one without the other
    static std::atomic<uint32_t> per_dev[64];
    constexpr auto kern = &k_sparse_vqe_rows_shared<NW, RPT, EPR, SSTRIDE, TE, DBG>;
    constexpr size_t slots = (size_t)RPT * EPR * NW * 64;   // the packed tables: coefficients, then 16-bit offsets (sparse_pack.hpp)
    const double *hc = (const double *)h->d_sp_hpack.p;
    const uint16_t *ho = (const uint16_t *)(hc + slots);
    if (int rc = lds_opt_in<kern>(h, LDS_WG_MAX)) return rc;
    uint32_t pd = per_dev[h->device & 63].load(std::memory_order_relaxed);
    if ((pd >> 8) != smem) {
        int n = 0;
        HIPC(h, hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kern, NW * 64, smem));
        pd = (uint32_t)smem << 8 | (uint32_t)std::min(std::max(n, 1), 32 / NW);
        per_dev[h->device & 63].store(pd, std::memory_order_relaxed);
    }
    const int per_cu = (int)(pd & 255u);
    handle_num_cus(h);
    // persistent: as many workgroups as the chip holds at once, each walks work items of 2 NW evaluations
    const int grid = (int)std::min<int64_t>((R.B + NS - 1) / NS, (int64_t)h->num_cus * per_cu);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(NW * 64), smem, h->stream, R, h->cur_theta, (const SmallRot *)h->d_sp_prim.p,
                       (const uint64_t *)h->d_sp_rows.p, h->sp_nrows4, hc, ho, h->cur_energies);
    HIPC(h, hipGetLastError());
    return OVQE_OK;
}

// Instance K of the workgroup geometry.  *taken = false: it does not hold this program (nothing launched): more entries than
// its capacity criterion, a support beyond its stride, entries that do not pack into its pieces (all three decided with the
// tables: build_sparse_program packed for instance sp_pack_inst), or states + cos/sin tables beyond the LDS of half a CU.
template <int K>
int launch_rows_shared(ovqe_handle h, const SparseArgs &R, bool *taken) {
    constexpr SharedInstance I = SHARED_INSTANCES[K];
    constexpr int NW = I.nw, RPT = I.rpt, EPR = I.epr, SSTRIDE = I.sstride, TE = I.te;
    const size_t smem = sp_rows_shared_lds<NW, SSTRIDE>(R.ntab).bytes;
    *taken = h->sp_pack_inst == K && R.nent >= 1 && R.nent <= NW * 64 * I.ept && (size_t)R.mpad * sizeof(double) <= (size_t)SSTRIDE &&
             smem <= LDS_TWO_PER_CU;
    if (!*taken) return OVQE_OK;
#ifdef OVQE_TESTING
    switch (h->opt_sparse_dbg) {
    case 1: return launch_rows_shared_dbg<NW, RPT, EPR, SSTRIDE, TE, 1>(h, R, smem);
    case 2: return launch_rows_shared_dbg<NW, RPT, EPR, SSTRIDE, TE, 2>(h, R, smem);
    case 3: return launch_rows_shared_dbg<NW, RPT, EPR, SSTRIDE, TE, 3>(h, R, smem);
    case 4: return launch_rows_shared_dbg<NW, RPT, EPR, SSTRIDE, TE, 4>(h, R, smem);
    case 5: return launch_rows_shared_dbg<NW, RPT, EPR, SSTRIDE, TE, 5>(h, R, smem);
    default: break;
    }
#endif
    return launch_rows_shared_dbg<NW, RPT, EPR, SSTRIDE, TE, 0>(h, R, smem);
}

// the kernel arguments of the handle's compact program for a batch of B rows
SparseArgs sparse_args(ovqe_handle h, int64_t B) {
    SparseArgs A;
    A.m = h->sp_mp;
    A.mpad = (h->sp_mp + 1) & ~1;
    A.hf = h->sp_hf;
    A.K = h->K;
    A.nops = h->sp_nops;
    A.ntab = (int)h->srots.size();
    A.nent = h->sp_nent;
    A.npairs = (int)h->sp_npairs;
    A.B = B;
    A.constant = h->ham.constant;
    return A;
}

// on_device: theta / energies are device pointers (inputs already resident in HBM, results left there).  *done = false: no compact
// form fits this program's LDS budget (nothing was launched; the caller takes the other paths).
int run_sparse(ovqe_handle h, int64_t B, const double *theta, double *energies, bool on_device, bool *done) {
    *done = false;
    int rc = OVQE_OK;
    SparseArgs A = sparse_args(h, B);
    A.dbg = h->opt_sparse_dbg;
    int spw = h->opt_sparse_spw;
    if (spw != 1 && spw != 2 && spw != 4) spw = B >= 2048 ? 2 : 1;  // measured: 2 evaluations per wave is the sweet spot
    if (B <= 1024) spw = 1;
    while (spw > 1 && sp_vqe_lds(A, spw, false).bytes > 64 * 1024) spw >>= 1;
    // the workgroup form holds one cos/sin entry per distinct angle (at most 4094 of them, 64 KiB: its row tables exist only then)
    // and fits whatever the whole table takes; every other form holds the whole table
    const bool wg = B <= 256 && h->sp_nrows8 && h->opt_sparse_rows && h->opt_sparse_wg;
    if (!wg && sp_vqe_lds(A, spw, false).bytes > LDS_WG_BUDGET) {
        h->sp_forms |= SPF_DECLINED;
        return OVQE_OK;
    }
    const double *d_theta = theta;
    double *d_energies = energies;
    const bool zero_copy = !on_device && mapped_io(h, B);
    const bool poll = zero_copy && B <= 256 && h->opt_poll_result;   // (lone evaluations and finite-difference batches: microseconds)
    if (zero_copy) {
        std::memcpy(h->h_io, theta, (size_t)B * h->K * sizeof(double));
        if (poll) poll_arm(h->h_io + (size_t)B * h->K, B);
        d_theta = h->d_io;
        d_energies = h->d_io + (size_t)B * h->K;
    } else if (!on_device) {
        rc = ensure(h, h->d_theta, (size_t)B * std::max(1, h->K) * sizeof(double));
        if (!rc) rc = ensure(h, h->d_energies, (size_t)B * sizeof(double));
        if (rc) return rc;
        HIPC(h, hipMemcpyAsync(h->d_theta.p, theta, (size_t)B * h->K * sizeof(double), hipMemcpyHostToDevice, h->stream));
        d_theta = (const double *)h->d_theta.p;
        d_energies = (double *)h->d_energies.p;
    }
    h->cur_theta = d_theta;
    h->cur_energies = d_energies;
    const int64_t nwork = (B + spw - 1) / spw;
    const int grid = (int)std::min<int64_t>(nwork, 256 * 32);
    if (!zero_copy) HIPC(h, hipEventRecord(h->ev0, h->stream));
    // latency path: op table + pair words staged in LDS (one wave per evaluation, occupancy does not matter)
    const size_t staged = sp_vqe_lds(A, 1, true).bytes;
    if (wg) {
        // latency path: one evaluation per 1024-thread workgroup, at most one workgroup per CU (k_sparse_vqe_wg; measured: H2O
        // B = 1 / 141 32 / 37 us against 60 / 61 us with one wave per evaluation, B = 1024 129 against 115 us)
        SparseArgs R = A;
        R.mpad = (h->sp_mp + 128 + 1) & ~1;
        R.ntab = h->sp_nprim;
        const size_t smem = sp_rows_lds(R, 1).bytes;
        rc = lds_opt_in<&k_sparse_vqe_wg<1024, 10>>(h, LDS_WG_BUDGET);
        if (rc) return rc;
        hipLaunchKernelGGL((k_sparse_vqe_wg<1024, 10>), dim3((unsigned)std::min<int64_t>(B, 1024)), dim3(1024), smem, h->stream, R, h->cur_theta,
                           (const SmallRot *)h->d_sp_prim.p, (const uint64_t *)h->d_sp_rows64.p, h->sp_nrows8, (const SpEntry *)h->d_sp_entries.p,
                           h->cur_energies);
        HIPC(h, hipGetLastError());
        h->sp_forms |= SPF_WG;
    }
    else if (B <= 1024 && staged <= 96 * 1024) {
        rc = launch_sparse<1, true>(h, A, grid, staged);
        h->sp_forms |= SPF_STAGED1;
    }
    else if (spw == 4) {
        rc = launch_sparse<4>(h, A, grid, sp_vqe_lds(A, 4, false).bytes);
        h->sp_forms |= SPF_PLAIN4;
    }
    else if (spw == 2 && h->sp_nrows4 && h->opt_sparse_rows) {
        SparseArgs R = A;
        R.mpad = (h->sp_mp + 64 + 1) & ~1;   // + the padded lanes' spare slots
        R.ntab = h->sp_nprim;                // one entry per distinct angle
        // batches that fill the chip: the workgroup geometry when one of its instances holds the program — a pure function of the
        // program and B; smaller instance first
        bool shared = false;
        if ((B >= SHARED_MIN_B && h->opt_sparse_shared) || h->opt_sparse_shared >= 2) {   // (2: the threshold sweep)
            if (!rc && !shared) {
                rc = launch_rows_shared<0>(h, R, &shared);
                if (shared) h->sp_forms |= SPG_SHARED_13;
            }
            if (!rc && !shared) {
                rc = launch_rows_shared<1>(h, R, &shared);
                if (shared) h->sp_forms |= SPG_SHARED_37;
            }
            if (rc) return rc;
        }
        if (!shared) {
#define OVQE_ROWS(DBG_)                                                                                                                       \
    do {                                                                                                                                      \
        rc = lds_opt_in<&k_sparse_vqe_rows<2, DBG_>>(h, LDS_WG_MAX);                                                                          \
        if (rc) return rc;                                                                                                                    \
        hipLaunchKernelGGL((k_sparse_vqe_rows<2, DBG_>), dim3(grid), dim3(64), sp_rows_lds(R, 2).bytes, h->stream, R, h->cur_theta,            \
                           (const SmallRot *)h->d_sp_prim.p, (const uint64_t *)h->d_sp_rows.p, h->sp_nrows4, (const SpEntry *)h->d_sp_entries.p, \
                           h->cur_energies);                                                                                                  \
    } while (0)
            switch (h->opt_sparse_dbg) {   // (measurement variants)
            case 1: OVQE_ROWS(1); break;
            case 2: OVQE_ROWS(2); break;
            case 3: OVQE_ROWS(3); break;
#ifdef OVQE_TESTING
            case 5: OVQE_ROWS(5); break;
#endif
            default: OVQE_ROWS(0);
            }
#undef OVQE_ROWS
            HIPC(h, hipGetLastError());
            h->sp_forms |= SPG_PER_WAVE;
        }
        h->sp_forms |= SPF_ROWS2;
    }
    else if (spw == 2) {
        rc = launch_sparse<2>(h, A, grid, sp_vqe_lds(A, 2, false).bytes);
        h->sp_forms |= SPF_PLAIN2;
    }
    else {
        rc = launch_sparse<1>(h, A, grid, sp_vqe_lds(A, 1, false).bytes);
        h->sp_forms |= SPF_PLAIN1;
    }
    if (rc) return rc;
    *done = true;
    if (zero_copy) {
        if (!poll || !poll_mapped_slots(h->h_io + (size_t)B * h->K, B)) HIPC(h, hipStreamSynchronize(h->stream));
        std::memcpy(energies, h->h_io + (size_t)B * h->K, (size_t)B * sizeof(double));
        h->last_batch_ms = 0.f;
        return OVQE_OK;
    }
    HIPC(h, hipEventRecord(h->ev1, h->stream));
    if (!on_device)
        HIPC(h, hipMemcpyAsync(energies, h->cur_energies, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    HIPC(h, hipEventElapsedTime(&h->last_batch_ms, h->ev0, h->ev1));
    return OVQE_OK;
}

// E and all K derivatives of one parameter vector on the compact support, one launch (k_sparse_grad).  *done = false: the
// program has no compact support or its tables do not fit one workgroup's LDS (the caller takes the other paths).
int run_sparse_gradient(ovqe_handle h, const double *theta, double *energy, double *grad, bool *done) {
    *done = false;
    if (!(h->opt_force_path == 0 || h->opt_force_path == 3) || !h->opt_sparse_grad || h->n_local > 16) return OVQE_OK;
    int rc = OVQE_OK;
    if (!h->sp_tried) {
        rc = build_sparse_program(h);
        if (rc) return rc;
    }
    if (!h->sp_valid) {
        h->sp_forms |= SPF_DECLINED;
        return OVQE_OK;
    }
    const SparseArgs A = sparse_args(h, 1);
    const size_t base = sp_grad_lds(A, false).bytes, staged = sp_grad_lds(A, true).bytes;
    if (base > LDS_WG_BUDGET) {
        h->sp_forms |= SPF_DECLINED;
        return OVQE_OK;
    }
    const bool stage = staged <= LDS_WG_BUDGET;
    const bool zero_copy = mapped_io(h, 2);   // theta [K] | energy | gradient [K] in the pinned, device-mapped buffer
    const double *d_theta;
    double *d_e, *d_g;
    if (zero_copy) {
        std::memcpy(h->h_io, theta, (size_t)h->K * sizeof(double));
        d_theta = h->d_io;
        d_e = h->d_io + h->K;
        d_g = h->d_io + h->K + 1;
    } else {
        rc = ensure(h, h->d_theta, (size_t)std::max(1, h->K) * sizeof(double));
        if (!rc) rc = ensure(h, h->d_energies, (size_t)(h->K + 1) * sizeof(double));
        if (rc) return rc;
        HIPC(h, hipMemcpyAsync(h->d_theta.p, theta, (size_t)h->K * sizeof(double), hipMemcpyHostToDevice, h->stream));
        d_theta = (const double *)h->d_theta.p;
        d_e = (double *)h->d_energies.p;
        d_g = d_e + 1;
    }
    bool launched = false;
    if (h->sp_nrows8 && h->opt_sparse_rows && h->opt_sparse_wg) {
        SparseArgs R = A;
        R.mpad = (h->sp_mp + 128 + 1) & ~1;
        R.ntab = h->sp_nprim;
        const size_t smem = sp_grad_wg_lds(R).bytes;
        rc = lds_opt_in<&k_sparse_grad_wg<1024, 10>>(h, LDS_WG_BUDGET);
        if (rc) return rc;
        if (smem <= LDS_WG_BUDGET) {
            hipLaunchKernelGGL((k_sparse_grad_wg<1024, 10>), dim3(1), dim3(1024), smem, h->stream, R, d_theta, (const SmallRot *)h->d_sp_prim.p,
                               (const uint64_t *)h->d_sp_rows64.p, h->sp_nrows8, (const SpEntry *)h->d_sp_entries.p, d_e, d_g);
            HIPC(h, hipGetLastError());
            h->sp_forms |= SPF_GRAD_WG;
            launched = true;
        }
    }
    if (!launched) {
        rc = launch_staged<&k_sparse_grad<true>, &k_sparse_grad<false>>(h, stage, 1u, stage ? staged : base, A, d_theta, (const SmallRot *)h->d_rots.p,
                                                                         (const SpOp *)h->d_sp_ops.p, (const uint32_t *)h->d_sp_pairs.p,
                                                                         (const SpEntry *)h->d_sp_entries.p, d_e, d_g);
        if (rc) return rc;
        h->sp_forms |= stage ? SPF_GRAD_STAGED : SPF_GRAD_PLAIN;
    }
    if (zero_copy) {
        HIPC(h, hipStreamSynchronize(h->stream));
        *energy = h->h_io[h->K];
        std::memcpy(grad, h->h_io + h->K + 1, (size_t)h->K * sizeof(double));
    } else {
        HIPC(h, hipMemcpyAsync(energy, d_e, sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIPC(h, hipMemcpyAsync(grad, d_g, (size_t)h->K * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIPC(h, hipStreamSynchronize(h->stream));
    }
    *done = true;
    return OVQE_OK;
}
