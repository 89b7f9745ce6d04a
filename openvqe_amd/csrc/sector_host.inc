// sector_host.inc — host side of the sector path (sv_sector.hpp); included by ovqe_sv.hip inside its anonymous namespace.
// Everything here is one-time table construction (on the device) plus the per-evaluation launch sequence.

// LDS the staged forms of the table builders (k_sec_pairs2, k_sec_hbuild) may take, key map included: a whole CU's budget behind the
// dense map, 60 KiB behind a tile's sorted keys
constexpr size_t sec_staged_budget(bool dense_map) { return dense_map ? LDS_WG_BUDGET : (size_t)60 * 1024; }

void free_buf(DevBuf &b) {
    release_block(b.p, b.cap);   // (kept for the running build's next allocations, else hipFree: DevBlockCache)
    b.p = nullptr;
    b.cap = 0;
}
void free_layout(SectorLayout &L) {
    free_buf(L.d_cid);
    free_buf(L.d_off);
    free_buf(L.d_src);
}
void free_hsweep(SectorHSweep &s) {
    free_layout(s.L);
    for (DevBuf *b : {&s.d_cbase, &s.d_clen, &s.d_cwords, &s.d_cvals, &s.d_dict, &s.d_xbase, &s.d_xlen, &s.d_xwords, &s.d_xvals, &s.d_order, &s.d_torder})
        free_buf(*b);
}
void free_sector(SectorEngine &E) {
    for (SectorSeg &s : E.segs) {
        free_layout(s.L);
        free_buf(s.d_tab0);
        free_buf(s.d_poff);
        free_buf(s.d_pairs);
        free_buf(s.d_srcpad);
        free_buf(s.d_dstpad);
        free_buf(s.d_wide);
        free_buf(s.d_rounds);
        free_buf(s.d_stream);
        free_buf(s.d_rowhdr);
        free_buf(s.d_rowinfo);
        free_buf(s.d_bdst);
        free_buf(s.d_torder);
        free_buf(s.d_regops);
        free_buf(s.d_reggw);
        free_buf(s.d_regsrc);
        free_buf(s.d_reggslot);
        free_buf(s.d_regoslot);
    }
    free_buf(E.d_regmap);
    free_buf(E.d_regtab);
    E.nregtab = 0;
    E.regular = false;
    E.pad_elems = 0;
    for (SectorHSweep &s : E.hs) free_hsweep(s);
    E.segs.clear();
    E.hs.clear();
    for (DevBuf *b : {&E.d_sup, &E.d_buf[0], &E.d_buf[1], &E.d_hdesc, &E.d_flag, &E.d_lam[0], &E.d_lam[1], &E.d_w, &E.d_wpart,
                      &E.d_bbuf[0], &E.d_bbuf[1], &E.d_brp, &E.d_benergies})
        free_buf(*b);
    for (hipEvent_t &e : E.ev) {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
    E.last_circuit_ms = E.last_expect_ms = 0.f;
    E.h_stream_bytes = 0;
    E.valid = false;
    E.K = 0;
    E.npairs = E.nnz = 0;
    E.bytes = 0;
}

// the tables of a SMALL engine go to the handle's kept blocks instead of back to the driver (some 200 buffers: hipFree synchronises and
// unmaps, 4-6 ms in all; the next build — an ADAPT run rebuilds every macro-iteration — takes most of its allocations from them).  Large
// engines are freed for real: their successor sizes itself from hipMemGetInfo.
void free_sector_kept(ovqe_handle h, SectorEngine &E) {
    if (E.bytes == 0 || E.bytes > ((size_t)192 << 20) || DevBlockCache::current) {
        free_sector(E);
        return;
    }
    DevBlockScope kept_blocks(h->kept_blocks);
    free_sector(E);
}

struct SectorScratch {   // build-time buffers
    DevBuf keys_in, keys, ids_in, inv, inv_circ, temp, cnt, cnt2, rank, ops, pats, groups, lterms, ecnt, ecnt2, maxn, dkeys, dsorted, dunique, wbase;
    ~SectorScratch() {
        for (DevBuf *b : {&keys_in, &keys, &ids_in, &inv, &inv_circ, &temp, &cnt, &ops, &pats, &groups, &lterms, &ecnt, &ecnt2, &maxn, &dkeys,
                          &dsorted, &dunique, &cnt2, &rank, &wbase})
            free_buf(*b);
    }
};

// support of the real state in h->state, ascending, on the device
int sector_support(ovqe_handle h, SectorEngine &E, std::vector<uint32_t> &sup_host) {
    const uint64_t per_block = 256ull * SEC_NZ_PER_THREAD;
    const unsigned nb = (unsigned)((h->namps + per_block - 1) / per_block);
    DevBuf d_cnt;
    int rc = ensure(h, d_cnt, (size_t)nb * sizeof(uint32_t));
    if (rc) return rc;
    hipLaunchKernelGGL(k_sec_count_nz, dim3(nb), dim3(256), 0, h->stream, (const double *)h->state, h->namps, (uint32_t *)d_cnt.p);
    std::vector<uint32_t> cnt(nb);
    hipError_t e = hipMemcpyAsync(cnt.data(), d_cnt.p, (size_t)nb * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        free_buf(d_cnt);
        return fail(h, OVQE_ERR_HIP, hipGetErrorString(e));
    }
    uint64_t total = 0;
    for (unsigned b = 0; b < nb; ++b) {
        const uint32_t c = cnt[b];
        cnt[b] = (uint32_t)total;
        total += c;
    }
    E.K = 0;
    if (total == 0 || total * (uint64_t)std::max(h->opt_sector_sparsity, 2) > h->namps || total > 0x7ffffff0ull) {   // not sparse enough to pay off (or beyond 32-bit positions)
        free_buf(d_cnt);
        return OVQE_OK;
    }
    rc = upload(h, d_cnt, cnt.data(), (size_t)nb * sizeof(uint32_t));
    if (!rc) rc = ensure(h, E.d_sup, (size_t)total * sizeof(uint32_t));
    if (rc) {
        free_buf(d_cnt);
        return rc;
    }
    hipLaunchKernelGGL(k_sec_fill_nz, dim3(nb), dim3(256), 0, h->stream, (const double *)h->state, h->namps,
                       (const uint32_t *)d_cnt.p, (uint32_t *)E.d_sup.p);
    sup_host.resize(total);
    e = hipMemcpyAsync(sup_host.data(), E.d_sup.p, (size_t)total * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    free_buf(d_cnt);
    if (e != hipSuccess) return fail(h, OVQE_ERR_HIP, hipGetErrorString(e));
    E.K = (uint32_t)total;
    return OVQE_OK;
}

// the support sorted for the tile bit set smask: L.d_cid / L.d_off; W.keys (sorted keys) and W.inv (canonical id -> position)
// stay valid until the next call
int sector_layout(ovqe_handle h, SectorEngine &E, SectorScratch &W, uint32_t smask, int M, SectorLayout &L) {
    const uint32_t K = E.K;
    const uint32_t all = (uint32_t)(h->namps - 1ull);
    L.smask = smask;
    L.M = M;
    L.ntiles = (uint32_t)(h->namps >> M);
    const size_t kb = (size_t)K * sizeof(uint32_t);
    int rc = ensure(h, W.keys_in, kb);
    if (!rc) rc = ensure(h, W.keys, kb);
    if (!rc) rc = ensure(h, W.ids_in, kb);
    if (!rc) rc = ensure(h, W.inv, kb);
    if (!rc) rc = ensure(h, W.maxn, 256);
    if (!rc) rc = ensure(h, L.d_cid, kb);
    if (!rc) rc = ensure(h, L.d_off, ((size_t)L.ntiles + 1) * sizeof(uint32_t));
    if (rc) return rc;
    const unsigned g = (K + 255u) / 256u;
    hipLaunchKernelGGL(k_sec_keys, dim3(g), dim3(256), 0, h->stream, (const uint32_t *)E.d_sup.p, K, smask, all & ~smask, M,
                       (uint32_t *)W.keys_in.p, (uint32_t *)W.ids_in.p);
    size_t tb = 0;
    hipError_t e = hipcub::DeviceRadixSort::SortPairs(nullptr, tb, (const uint32_t *)W.keys_in.p, (uint32_t *)W.keys.p,
                                                      (const uint32_t *)W.ids_in.p, (uint32_t *)L.d_cid.p, (int)K, 0, h->n_local,
                                                      h->stream);
    if (e != hipSuccess) return fail(h, OVQE_ERR_HIP, std::string("radix sort (size query): ") + hipGetErrorString(e));
    rc = ensure(h, W.temp, tb);
    if (rc) return rc;
    tb = W.temp.cap;
    e = hipcub::DeviceRadixSort::SortPairs(W.temp.p, tb, (const uint32_t *)W.keys_in.p, (uint32_t *)W.keys.p,
                                           (const uint32_t *)W.ids_in.p, (uint32_t *)L.d_cid.p, (int)K, 0, h->n_local, h->stream);
    if (e != hipSuccess) return fail(h, OVQE_ERR_HIP, std::string("radix sort: ") + hipGetErrorString(e));
    hipLaunchKernelGGL(k_sec_offsets, dim3(g), dim3(256), 0, h->stream, (const uint32_t *)W.keys.p, K, M, L.ntiles, (uint32_t *)L.d_off.p);
    hipLaunchKernelGGL(k_sec_inverse, dim3(g), dim3(256), 0, h->stream, (const uint32_t *)L.d_cid.p, K, (uint32_t *)W.inv.p);
    HIPC(h, hipMemsetAsync(W.maxn.p, 0, sizeof(uint32_t), h->stream));
    hipLaunchKernelGGL(k_sec_max_tile, dim3(std::min(1024u, (L.ntiles + 255u) / 256u)), dim3(256), 0, h->stream,
                       (const uint32_t *)L.d_off.p, L.ntiles, (uint32_t *)W.maxn.p);
    HIPC(h, hipGetLastError());
    HIPC(h, hipMemcpyAsync(&L.max_tile, W.maxn.p, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    return OVQE_OK;
}

// d_src of L: where every entry of L sits in the layout whose inverse map is inv_prev
int sector_compose(ovqe_handle h, SectorEngine &E, SectorLayout &L, const DevBuf &inv_prev) {
    int rc = ensure(h, L.d_src, (size_t)E.K * sizeof(uint32_t));
    if (rc) return rc;
    hipLaunchKernelGGL(k_sec_compose, dim3((E.K + 255u) / 256u), dim3(256), 0, h->stream, (const uint32_t *)L.d_cid.p,
                       (const uint32_t *)inv_prev.p, E.K, (uint32_t *)L.d_src.p);
    HIPC(h, hipGetLastError());
    return OVQE_OK;
}

// Per-wave streams of one sweep (third form of the sweep kernel, sv_sector.hpp): the op list cut into runs whose mixing masks leave
// log2(waves) tile bits untouched, rows counted per (tile, wave, op) on the device, offsets on the host, words filled on the device.
// A sweep whose runs would hold fewer than two ops on average keeps the second form (sg.nruns = 0).
int build_wave_streams(ovqe_handle h, SectorEngine &E, SectorScratch &W, SectorSeg &sg, const std::vector<SecBuildOp> &sops,
                       uint32_t maxp, uint64_t S, int M, int sb) {
    (void)W;
    sg.nruns = 0;
    if (sg.nops == 0 || sg.L.max_tile > 0x7ffeu) return OVQE_OK;
    // the streams are walked by 1024-thread workgroups, one per tile (run_sector_circuit): registers with three or more tiles per CU take
    // 512-thread workgroups of the second form, three to a CU, and so does a handle told to use another workgroup size
    if ((h->opt_sector_threads != 0 && h->opt_sector_threads != 1024) || (h->opt_sector_threads == 0 && sg.L.ntiles >= 768u))
        return OVQE_OK;
    int NW = h->opt_sector_stream_waves;
    if (NW != 1 && NW != 2 && NW != 4 && NW != 8 && NW != 16) NW = sec_stream_wave_count((double)maxp / (double)sg.nops, SEC_STREAM_WAVES);
    if (NW == 0) return OVQE_OK;
    std::vector<SecWaveRun> runs;
    if (!sec_plan_wave_runs(sops, S, M, NW, SEC_STREAM_CLASS_BITS, runs)) return OVQE_OK;   // (an op wider than a run)
    const int nruns = (int)runs.size();
    if (nruns + 1 > 64 || 2 * nruns > sg.nops) return OVQE_OK;
    const uint32_t nt = sg.L.ntiles;
    DevBuf d_runs, d_oprows, d_rowoff, d_wof, d_arranged;
    auto done = [&](int rc) {
        free_buf(d_arranged);
        free_buf(d_runs);
        free_buf(d_oprows);
        free_buf(d_rowoff);
        free_buf(d_wof);
        if (rc == OVQE_ERR_ALLOC) {
            // the streams are an optional extra on top of the second form's tables: a failed allocation (they hold their words twice
            // while the lanes are arranged) leaves the sweep on the second form instead of failing the whole table build
            free_buf(sg.d_stream);
            free_buf(sg.d_rowhdr);
            free_buf(sg.d_rowinfo);
            (void)hipGetLastError();
            sg.nruns = 0;
            return OVQE_OK;
        }
        return rc;
    };
    int rc = upload(h, d_runs, runs.data(), runs.size() * sizeof(SecWaveRun));
    if (!rc) rc = ensure(h, d_oprows, (size_t)nt * NW * sg.nops * sizeof(uint32_t));
    if (!rc) rc = ensure(h, d_wof, (size_t)nt * nruns * (1u << SEC_STREAM_CLASS_BITS));
    if (rc) return done(rc);
    const uint32_t pcap = (std::max(sg.L.max_tile, 1u) + 3u) & ~3u;
    const size_t smem = sec_wave_plan_lds(pcap, sg.nops, NW).bytes;
    if (smem > 64 * 1024) return done(OVQE_OK);   // (a sweep of hundreds of ops over 16 waves: the second form serves it)
    hipLaunchKernelGGL((k_sec_wave_plan<false>), dim3(nt), dim3(256), smem, h->stream, (const uint32_t *)E.d_sup.p, (const uint32_t *)sg.L.d_cid.p,
                       (const uint32_t *)sg.L.d_off.p, (const uint32_t *)sg.d_pairs.p, (const uint32_t *)sg.d_poff.p, sg.nops,
                       (const int32_t *)sg.d_tab0.p, sg.rot0, (const SecWaveRun *)d_runs.p, nruns, sb, NW, pcap, (uint32_t *)d_oprows.p,
                       (const uint32_t *)nullptr, (uint8_t *)d_wof.p, (uint32_t *)nullptr, (uint16_t *)nullptr);
    if (hipGetLastError() != hipSuccess) return done(fail(h, OVQE_ERR_HIP, "sector: stream plan launch"));
    std::vector<uint32_t> oprows((size_t)nt * NW * sg.nops), rowoff((size_t)nt * NW * (sg.nops + 1)), rowinfo((size_t)nt * NW * (nruns + 1));
    if (hipMemcpyAsync(oprows.data(), d_oprows.p, oprows.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
        hipStreamSynchronize(h->stream) != hipSuccess)
        return done(fail(h, OVQE_ERR_HIP, "sector: stream plan"));
    uint64_t rows = 0;
    for (size_t q = 0; q < (size_t)nt * NW; ++q) {
        for (int o = 0; o < sg.nops; ++o) {
            rowoff[q * (sg.nops + 1) + o] = (uint32_t)rows;
            rows += oprows[q * sg.nops + o];
        }
        rowoff[q * (sg.nops + 1) + sg.nops] = (uint32_t)rows;
        for (int r = 0; r <= nruns; ++r) rowinfo[q * (nruns + 1) + r] = rowoff[q * (sg.nops + 1) + (r ? runs[r - 1].op_end : 0)];
    }
    if (rows * 64ull > 0xfffffff0ull) return done(OVQE_OK);
    // the streams are an extra on top of the tables the second form needs: they go first when the budget is short (they take their
    // words twice while the lanes are being arranged)
    if (E.budget && E.bytes + (size_t)(rows + 2 * SEC_STREAM_G) * 64u * sizeof(uint32_t) * 2u > E.budget) return done(OVQE_OK);
    const size_t words = ((size_t)rows + 2 * SEC_STREAM_G) * 64u, hdrs = (size_t)rows + 4 * SEC_STREAM_G;   // (the sweep kernel loads two batches past a wave's last row)
    rc = upload(h, d_rowoff, rowoff.data(), rowoff.size() * sizeof(uint32_t));
    if (!rc) rc = upload(h, sg.d_rowinfo, rowinfo.data(), rowinfo.size() * sizeof(uint32_t));
    if (!rc) rc = ensure(h, sg.d_stream, words * sizeof(uint32_t));
    if (!rc) rc = ensure(h, sg.d_rowhdr, hdrs * sizeof(uint16_t));
    if (rc) return done(rc);
    if (hipMemsetAsync(sg.d_stream.p, 0xff, words * sizeof(uint32_t), h->stream) != hipSuccess ||
        hipMemsetAsync(sg.d_rowhdr.p, 0, hdrs * sizeof(uint16_t), h->stream) != hipSuccess)
        return done(fail(h, OVQE_ERR_HIP, "sector: stream tables"));
    hipLaunchKernelGGL((k_sec_wave_plan<true>), dim3(nt), dim3(256), smem, h->stream, (const uint32_t *)E.d_sup.p, (const uint32_t *)sg.L.d_cid.p,
                       (const uint32_t *)sg.L.d_off.p, (const uint32_t *)sg.d_pairs.p, (const uint32_t *)sg.d_poff.p, sg.nops,
                       (const int32_t *)sg.d_tab0.p, sg.rot0, (const SecWaveRun *)d_runs.p, nruns, sb, NW, pcap, (uint32_t *)nullptr,
                       (const uint32_t *)d_rowoff.p, (uint8_t *)d_wof.p, (uint32_t *)sg.d_stream.p, (uint16_t *)sg.d_rowhdr.p);
    if (hipGetLastError() != hipSuccess) return done(fail(h, OVQE_ERR_HIP, "sector: stream fill"));
    if (h->opt_sector_stream_arrange && rows > 0) {   // lanes of every row chosen for the LDS banks
        rc = ensure(h, d_arranged, words * sizeof(uint32_t));
        if (rc) return done(rc);
        if (hipMemsetAsync(d_arranged.p, 0xff, words * sizeof(uint32_t), h->stream) != hipSuccess)
            return done(fail(h, OVQE_ERR_HIP, "sector: stream tables"));
        hipLaunchKernelGGL(k_sec_row_arrange, dim3((unsigned)((rows + 255u) / 256u)), dim3(256), 0, h->stream, (const uint32_t *)sg.d_stream.p,
                           (uint32_t *)d_arranged.p, rows, sb);
        if (hipGetLastError() != hipSuccess) return done(fail(h, OVQE_ERR_HIP, "sector: stream arrange"));
        std::swap(sg.d_stream, d_arranged);
    }
    if (hipStreamSynchronize(h->stream) != hipSuccess) return done(fail(h, OVQE_ERR_HIP, "sector: stream fill"));
#ifdef OVQE_TESTING
    if (h->opt_sector_debug & 8) {   // rows by fill and by distinct patterns (measurement)
        std::vector<uint32_t> st((size_t)rows * 64u);
        if (rows && hipMemcpy(st.data(), sg.d_stream.p, st.size() * 4, hipMemcpyDeviceToHost) == hipSuccess) {
            uint64_t npat[5] = {0, 0, 0, 0, 0}, lanes = 0, orph = 0;
            for (uint64_t r = 0; r < rows; ++r) {
                uint32_t seen = 0;
                for (int l = 0; l < 64; ++l) {
                    const uint32_t w = st[r * 64 + l];
                    if (w == 0xffffffffu) continue;
                    ++lanes;
                    if (((w >> sb) & ((1u << sb) - 1u)) == ((1u << sb) - 1u)) ++orph;
                    seen |= 1u << (((w & 0x7fffffffu) >> (2 * sb)) & 31u);
                }
                npat[std::min(__builtin_popcount(seen), 4)]++;
            }
            fprintf(stderr, "ovqe: streams of a sweep: %d ops in %d runs, %d waves, %llu rows, fill %.2f, rows by distinct patterns 0/1/2/3/4+: %llu %llu %llu %llu %llu, %llu orphan words\n",
                    sg.nops, nruns, NW, (unsigned long long)rows, (double)lanes / (64.0 * (double)rows), (unsigned long long)npat[0], (unsigned long long)npat[1],
                    (unsigned long long)npat[2], (unsigned long long)npat[3], (unsigned long long)npat[4], (unsigned long long)orph);
        }
    }
#endif
    sg.nruns = nruns;
    sg.stream_waves = NW;
    sg.stream_rows = rows;
    E.bytes += words * sizeof(uint32_t) + hdrs * sizeof(uint16_t) + rowinfo.size() * sizeof(uint32_t);
    return done(OVQE_OK);
}

int sector_tile_bits(ovqe_handle h) {
    if (h->opt_sector_bits > 0) return std::max(6, std::min({h->opt_sector_bits, h->n_local - 1, 20}));
    return std::max(8, std::min(16, h->n_local - 8));   // 256 tiles up to 24 qubits, 2^16-amplitude dense tiles beyond
}

// "sector_debug" bit 1 (value 2): say on stderr why a program was left to the dense kernels
#define SEC_DECLINE(msg)                                                                          \
    do {                                                                                          \
        if (h->opt_sector_debug & 2) fprintf(stderr, "ovqe: sector path declined: %s\n", msg);   \
        return OVQE_OK;                                                                           \
    } while (0)
// ---- <H> restricted to the support E.d_sup (E.K entries, ascending), vectors in the order whose inverse map (canonical id ->
// position) is W.inv_circ: greedy cover of the x-groups by tile bit sets (grow_tile_set(), sv_cover_host.hpp), then the restricted
// Hamiltonian of every (sweep, tile).  E.M = the tile bits to start from; E.bytes = what the engine holds so far.
int build_sector_h(ovqe_handle h, SectorEngine &E, SectorScratch &W, size_t budget) {
    const uint32_t K = E.K;
    int rc = OVQE_OK;
    const HamDev &H = h->ham;
    const int G = (int)H.groups.size();
    // Without the <H> tables (budget, or an x-group wider than a tile) the engine still serves the circuit; <H> is then
    // evaluated by the compact cover (sv_tile.hpp) from the canonical compact state.
    E.h_tables = h->opt_sector_h != 0;
    auto drop_h = [&]() {
        for (SectorHSweep &s : E.hs) free_hsweep(s);
        E.hs.clear();
        E.nnz = 0;
        E.h_tables = false;
    };
    const size_t circuit_bytes = E.bytes;
    int maxw = 0;
    for (int g = 0; g < G; ++g) {
        maxw = std::max(maxw, __builtin_popcountll(H.groups[g].x));
        if (H.groups[g].x > 0xffffffffull) E.h_tables = false;
    }
    // a first guess before any table is built: about a third of the (entry, x-group) pairs carry a matrix element, half of
    // them are kept (pairs counted once), 4 bytes each
    if ((double)K * G * 0.15 * 4.0 > 2.0 * (double)budget) E.h_tables = false;
    struct HPlan {
        uint64_t S;
        std::vector<SecGroup> groups;
    };
    std::vector<HPlan> plan;
    auto make_plan = [&](int M) {
        plan.clear();
        std::vector<char> covered(G, 0);
        int remaining = G;
        while (remaining > 0) {
            std::vector<uint64_t> uncovered;
            for (int g = 0; g < G; ++g)
                if (!covered[g]) uncovered.push_back(H.groups[g].x);
            const uint64_t S = grow_tile_set(uncovered, 0, M, h->n_local);
            // element offsets of a sweep are 32-bit: a bit set with many x-groups on a large support becomes several
            // sweeps (same tiles, the groups shared out)
            const size_t gmax = std::max<size_t>(1, (size_t)(3.9e9 / (double)K));
            plan.push_back(HPlan{S, {}});
            bool any = false;
            for (int g = 0; g < G; ++g) {
                if (covered[g] || (H.groups[g].x & ~S)) continue;
                covered[g] = 1;
                --remaining;
                any = true;
                if (plan.back().groups.size() >= gmax) plan.push_back(HPlan{S, {}});
                plan.back().groups.push_back(SecGroup{H.groups[g].x, H.groups[g].t0, H.groups[g].t1});
            }
            if (!any) return false;
        }
        return true;
    };
    // tile bits of <H>: the circuit's, lowered until no tile exceeds the 13-bit slots / the LDS of the lambda kernel
    int Mh = 0;
    if (E.h_tables) {
        Mh = E.M;
        if (h->opt_sector_h_bits > 0) Mh = std::max(4, std::min(h->opt_sector_h_bits, h->n_local - 1));
        for (;; --Mh) {
            if (Mh < std::max(maxw, 4)) {
                E.h_tables = false;
                break;
            }
            if (!make_plan(Mh)) return fail(h, OVQE_ERR_INVALID, "internal: sector cover made no progress");
            bool fits = true;
            SectorLayout probe;
            for (const HPlan &pl : plan) {
                if (&pl != &plan[0] && pl.S == (&pl)[-1].S) continue;   // same tiles as the previous sweep
                rc = sector_layout(h, E, W, (uint32_t)pl.S, Mh, probe);
                if (rc) break;
                if (probe.max_tile > SEC_HTILE_LDS_CAP) {
                    fits = false;
                    break;
                }
            }
            free_layout(probe);
            if (rc) return rc;
            if (fits) break;
        }
    }
    E.Mh = Mh;
    E.h_max_tile = 0;
    E.h_max_dict = 0;
    constexpr int NTB = 1024;   // rows per tile run to thousands: one workgroup per tile needs the threads
    for (size_t ip = 0; E.h_tables && ip < plan.size(); ++ip) {
        const uint64_t S = plan[ip].S;
        const std::vector<SecGroup> &sg = plan[ip].groups;
        E.hs.emplace_back();
        SectorHSweep &hw = E.hs.back();
        rc = sector_layout(h, E, W, (uint32_t)S, Mh, hw.L);
        const size_t nsl = (size_t)hw.L.ntiles * SEC_HSLICES;
        if (!rc) rc = sector_compose(h, E, hw.L, W.inv_circ);
        // the sweep's x-groups and their terms as the 16-byte records k_sec_hbuild stages in LDS (terms with an odd number of Y dropped)
        std::vector<SecGroupL> gl;
        std::vector<SecTermL> tl;
        gl.reserve(sg.size());
        for (const SecGroup &g0 : sg) {
            SecGroupL r;
            r.x = (uint32_t)g0.x;
            r.lx = extract_bits(g0.x, S);
            r.t0 = (uint32_t)tl.size();
            for (int t = g0.t0; t < g0.t1; ++t) {
                const HTerm &ht = H.terms[t];
                if (__builtin_popcountll(g0.x & ht.z) & 1) continue;
                tl.push_back(SecTermL{(uint32_t)ht.z, 0u, ht.cr});
            }
            r.t1 = (uint32_t)tl.size();
            gl.push_back(r);
        }
        if (tl.empty()) tl.push_back(SecTermL{0u, 0u, 0.0});   // (never referenced: an upload needs a source)
        if (!rc) rc = upload(h, W.groups, gl.data(), gl.size() * sizeof(SecGroupL));
        if (!rc) rc = upload(h, W.lterms, tl.data(), tl.size() * sizeof(SecTermL));
        for (DevBuf *b : {&hw.d_cbase, &hw.d_clen, &hw.d_xbase, &hw.d_xlen, &W.cnt, &W.cnt2})
            if (!rc) rc = ensure(h, *b, (nsl + 1) * sizeof(uint32_t));
        if (!rc) rc = ensure(h, W.ecnt, ((size_t)K + 1) * sizeof(uint32_t));
        if (!rc) rc = ensure(h, W.ecnt2, ((size_t)K + 1) * sizeof(uint32_t));
        if (rc) return rc;
        HIPC(h, hipMemsetAsync(W.cnt.p, 0, (nsl + 1) * sizeof(uint32_t), h->stream));
        HIPC(h, hipMemsetAsync(W.cnt2.p, 0, (nsl + 1) * sizeof(uint32_t), h->stream));
        const bool dense_map = Mh <= 16;
        const size_t map_bytes = sec_map_bytes(dense_map, Mh, hw.L.max_tile, true);
        const int staged = sec_hbuild_lds(map_bytes, (int)gl.size(), (int)tl.size(), true).bytes <= sec_staged_budget(dense_map) ? 1 : 0;
        const size_t smem_h = sec_hbuild_lds(map_bytes, (int)gl.size(), (int)tl.size(), staged != 0).bytes;
        rc = lds_opt_in<&k_sec_hbuild<false, NTB, true>, &k_sec_hbuild<true, NTB, true>>(h, SEC_LDS_MAX);
        if (rc) return rc;
#define OVQE_HBUILD(FILL, DENSE, ...)                                                                                      \
    hipLaunchKernelGGL((k_sec_hbuild<FILL, NTB, DENSE>), dim3(hw.L.ntiles), dim3(NTB), smem_h, h->stream,                    \
                       (const uint32_t *)E.d_sup.p, (const uint32_t *)W.keys.p, (const uint32_t *)hw.L.d_cid.p,             \
                       (const uint32_t *)hw.L.d_off.p, Mh, (uint32_t)map_bytes, (const SecGroupL *)W.groups.p, (int)gl.size(),  \
                       (const SecTermL *)W.lterms.p, (int)tl.size(), staged, __VA_ARGS__)
        if (dense_map)
            OVQE_HBUILD(false, true, (uint32_t *)W.ecnt.p, (uint32_t *)W.ecnt2.p, (const uint32_t *)nullptr, (const uint32_t *)nullptr,
                        (const uint32_t *)nullptr, (const uint32_t *)nullptr, (const uint16_t *)nullptr, (uint32_t *)nullptr,
                        (double *)nullptr, (uint32_t *)nullptr, (double *)nullptr);
        else
            OVQE_HBUILD(false, false, (uint32_t *)W.ecnt.p, (uint32_t *)W.ecnt2.p, (const uint32_t *)nullptr, (const uint32_t *)nullptr,
                        (const uint32_t *)nullptr, (const uint32_t *)nullptr, (const uint16_t *)nullptr, (uint32_t *)nullptr,
                        (double *)nullptr, (uint32_t *)nullptr, (double *)nullptr);
        rc = ensure(h, hw.d_order, ((size_t)K + 1) * sizeof(uint16_t));
        if (!rc) rc = ensure(h, W.rank, ((size_t)K + 1) * sizeof(uint16_t));
        if (rc) return rc;
        {
            uint32_t P = 64;
            while (P < hw.L.max_tile) P <<= 1;
            hipLaunchKernelGGL((k_sec_row_order<256>), dim3(hw.L.ntiles), dim3(256), (size_t)P * sizeof(uint32_t), h->stream,
                               (const uint32_t *)hw.L.d_off.p, (const uint32_t *)W.ecnt.p, (const uint32_t *)W.ecnt2.p,
                               (uint16_t *)hw.d_order.p, (uint16_t *)W.rank.p);
        }
        hipLaunchKernelGGL(k_sec_slice_len, dim3(hw.L.ntiles), dim3(256), 0, h->stream, (const uint32_t *)hw.L.d_off.p,
                           (const uint16_t *)hw.d_order.p, (const uint32_t *)W.ecnt.p, (const uint32_t *)W.ecnt2.p, (uint32_t *)hw.d_clen.p, (uint32_t *)hw.d_xlen.p,
                           (uint32_t *)W.cnt.p, (uint32_t *)W.cnt2.p);
        HIPC(h, hipGetLastError());
        uint32_t totals[2] = {0, 0};
        for (int which = 0; which < 2; ++which) {
            const uint32_t *cnt = (const uint32_t *)(which ? W.cnt2.p : W.cnt.p);
            uint32_t *base = (uint32_t *)(which ? hw.d_xbase.p : hw.d_cbase.p);
            size_t tb = 0;
            hipError_t e = hipcub::DeviceScan::ExclusiveSum(nullptr, tb, cnt, base, (int)(nsl + 1), h->stream);
            if (e != hipSuccess) return fail(h, OVQE_ERR_HIP, std::string("scan (size query): ") + hipGetErrorString(e));
            rc = ensure(h, W.temp, tb);
            if (rc) return rc;
            tb = W.temp.cap;
            e = hipcub::DeviceScan::ExclusiveSum(W.temp.p, tb, cnt, base, (int)(nsl + 1), h->stream);
            if (e != hipSuccess) return fail(h, OVQE_ERR_HIP, std::string("scan: ") + hipGetErrorString(e));
            HIPC(h, hipMemcpyAsync(&totals[which], base + nsl, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
        }
        HIPC(h, hipStreamSynchronize(h->stream));
        const uint32_t ct = totals[0], xt = totals[1];   // padded element counts
        hw.nnz = (uint64_t)ct + xt;
        E.nnz += hw.nnz;
        E.bytes += (size_t)ct * 4 + (size_t)xt * 12 + (size_t)K * 4 + nsl * 16;
        E.h_stream_bytes += (size_t)ct * 4 + (size_t)xt * 12 + (size_t)K * (4 + 2 + 8) + nsl * 16;   // + src, order, gathered amplitudes
        if (E.bytes + (size_t)ct * 32 > budget) {   // (the coded stream's values and the sort buffers while building)
            drop_h();
            E.bytes = circuit_bytes;
            break;
        }
        rc = ensure(h, hw.d_cwords, (size_t)std::max<uint32_t>(ct, 1) * sizeof(uint32_t));
        if (!rc) rc = ensure(h, hw.d_cvals, (size_t)std::max<uint32_t>(ct, 1) * sizeof(double));
        if (!rc) rc = ensure(h, hw.d_xwords, (size_t)std::max<uint32_t>(xt, 1) * sizeof(uint32_t));
        if (!rc) rc = ensure(h, hw.d_xvals, (size_t)std::max<uint32_t>(xt, 1) * sizeof(double));
        if (rc) return rc;
        if (dense_map)
            OVQE_HBUILD(true, true, (uint32_t *)nullptr, (uint32_t *)nullptr, (const uint32_t *)hw.d_cbase.p, (const uint32_t *)hw.d_xbase.p,
                        (const uint32_t *)hw.d_clen.p, (const uint32_t *)hw.d_xlen.p, (const uint16_t *)W.rank.p,
                        (uint32_t *)hw.d_cwords.p, (double *)hw.d_cvals.p, (uint32_t *)hw.d_xwords.p, (double *)hw.d_xvals.p);
        else
            OVQE_HBUILD(true, false, (uint32_t *)nullptr, (uint32_t *)nullptr, (const uint32_t *)hw.d_cbase.p, (const uint32_t *)hw.d_xbase.p,
                        (const uint32_t *)hw.d_clen.p, (const uint32_t *)hw.d_xlen.p, (const uint16_t *)W.rank.p,
                        (uint32_t *)hw.d_cwords.p, (double *)hw.d_cvals.p, (uint32_t *)hw.d_xwords.p, (double *)hw.d_xvals.p);
#undef OVQE_HBUILD
        HIPC(h, hipGetLastError());
        // dictionary of the coded stream: sorted distinct magnitudes (the padding's 0 included)
        hw.ndict = 0;
        if (ct > 0 && h->opt_sector_dict) {
            rc = ensure(h, W.maxn, 256);
            if (rc) return rc;
            // first from a sample (every 16th value of a long stream), then — if k_sec_encode meets a magnitude the sample missed — from all
            uint32_t U = 0;
            bool coded = false, attempted = false;
            // ("sector_dict" 3, tests: a sample so thin that it misses magnitudes — the fall-back to all values at any size)
            for (uint32_t stride = h->opt_sector_dict == 3 ? 4096u : ((ct >= (1u << 20) && h->opt_sector_dict != 2) ? 16u : 1u);; stride = 1u) {
                const uint32_t m = (ct + stride - 1u) / stride;
                rc = ensure(h, W.dkeys, (size_t)m * sizeof(uint64_t));
                if (!rc) rc = ensure(h, W.dsorted, (size_t)m * sizeof(uint64_t));
                if (!rc) rc = ensure(h, W.dunique, (size_t)m * sizeof(uint64_t));
                if (rc) return rc;
                hipLaunchKernelGGL(k_sec_abs_keys, dim3((m + 255u) / 256u), dim3(256), 0, h->stream, (const double *)hw.d_cvals.p, ct, stride,
                                   (uint64_t *)W.dkeys.p);
                size_t tb = 0;
                hipError_t e = hipcub::DeviceRadixSort::SortKeys(nullptr, tb, (const uint64_t *)W.dkeys.p, (uint64_t *)W.dsorted.p, (int)m, 0, 64, h->stream);
                if (e != hipSuccess) return fail(h, OVQE_ERR_HIP, std::string("sort keys (size query): ") + hipGetErrorString(e));
                rc = ensure(h, W.temp, tb);
                if (rc) return rc;
                tb = W.temp.cap;
                e = hipcub::DeviceRadixSort::SortKeys(W.temp.p, tb, (const uint64_t *)W.dkeys.p, (uint64_t *)W.dsorted.p, (int)m, 0, 64, h->stream);
                if (e != hipSuccess) return fail(h, OVQE_ERR_HIP, std::string("sort keys: ") + hipGetErrorString(e));
                tb = 0;
                e = hipcub::DeviceSelect::Unique(nullptr, tb, (const uint64_t *)W.dsorted.p, (uint64_t *)W.dunique.p, (uint32_t *)W.maxn.p, (int)m, h->stream);
                if (e != hipSuccess) return fail(h, OVQE_ERR_HIP, std::string("unique (size query): ") + hipGetErrorString(e));
                rc = ensure(h, W.temp, tb);
                if (rc) return rc;
                tb = W.temp.cap;
                e = hipcub::DeviceSelect::Unique(W.temp.p, tb, (const uint64_t *)W.dsorted.p, (uint64_t *)W.dunique.p, (uint32_t *)W.maxn.p, (int)m, h->stream);
                if (e != hipSuccess) return fail(h, OVQE_ERR_HIP, std::string("unique: ") + hipGetErrorString(e));
                U = 0;
                HIPC(h, hipMemcpyAsync(&U, W.maxn.p, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
                HIPC(h, hipStreamSynchronize(h->stream));
                if (U < 1 || U > (uint32_t)SEC_DICT_MAX) {
                    if (stride == 1u || U > (uint32_t)SEC_DICT_MAX) break;   // (the whole stream has no fewer magnitudes than its sample)
                    continue;
                }
                rc = ensure(h, hw.d_dict, (size_t)U * sizeof(double));
                if (rc) return rc;
                HIPC(h, hipMemcpyAsync(hw.d_dict.p, W.dunique.p, (size_t)U * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
                HIPC(h, hipMemsetAsync((char *)W.maxn.p + 64, 0, sizeof(int), h->stream));
                attempted = true;
                hipLaunchKernelGGL(k_sec_encode, dim3((ct + 255u) / 256u), dim3(256), 0, h->stream, (uint32_t *)hw.d_cwords.p,
                                   (const double *)hw.d_cvals.p, ct, (const uint64_t *)hw.d_dict.p, (int)U, (int *)((char *)W.maxn.p + 64));
                HIPC(h, hipGetLastError());
                int miss = 0;
                HIPC(h, hipMemcpyAsync(&miss, (char *)W.maxn.p + 64, sizeof(int), hipMemcpyDeviceToHost, h->stream));
                HIPC(h, hipStreamSynchronize(h->stream));
                if (!miss) {
                    coded = true;
                    break;
                }
                if (stride == 1u) return fail(h, OVQE_ERR_INVALID, "internal: a coded value is missing from its own dictionary");
            }
            h->forms_used |= coded ? 0ull : (attempted ? SECF_H_SAMPLE_FAILED : SECF_H_OVERFLOW);
            if (!coded && attempted) {   // (the sample fitted a dictionary, the whole stream does not)
                hipLaunchKernelGGL(k_sec_words_slots, dim3((ct + 255u) / 256u), dim3(256), 0, h->stream, (uint32_t *)hw.d_cwords.p, ct);
                HIPC(h, hipGetLastError());
            }
            if (coded) {
                HIPC(h, hipStreamSynchronize(h->stream));
                free_buf(hw.d_cvals);
                hw.ndict = (int)U;
                if (h->opt_sector_h_pack && U <= (uint32_t)SEC_DICT_PACKED_MAX && (ct & 3u) == 0u && ct > 0) {
                    // a dictionary of up to 1023 magnitudes: the words have an empty top byte — the kernels stream 3 bytes per element
                    DevBuf packed;
                    rc = ensure(h, packed, ((size_t)(ct / 4u) * 3u + 1u) * sizeof(uint32_t));   // (+ 1: nothing past the last 12-byte group is ever out of bounds)
                    if (rc) return rc;
                    hipLaunchKernelGGL(k_sec_pack24, dim3((ct / 4u + 255u) / 256u), dim3(256), 0, h->stream, (const uint32_t *)hw.d_cwords.p, ct / 4u,
                                       (uint32_t *)packed.p);
                    HIPC(h, hipGetLastError());
                    HIPC(h, hipStreamSynchronize(h->stream));
                    std::swap(hw.d_cwords, packed);
                    free_buf(packed);
                    hw.packed = 1;
                    h->forms_used |= SECF_H_PACKED;
                    E.bytes -= std::min(E.bytes, (size_t)ct);
                    E.h_stream_bytes -= std::min(E.h_stream_bytes, (size_t)ct);
                }
                if (!hw.packed) h->forms_used |= SECF_H_DICT;
            }
        } else if (ct > 0) {
            h->forms_used |= SECF_H_NO_DICT;
        }
        if (!hw.ndict) {   // the coded stream keeps its explicit values
            E.bytes += (size_t)ct * 8;
            E.h_stream_bytes += (size_t)ct * 8;
        }
        HIPC(h, hipStreamSynchronize(h->stream));
        E.h_max_tile = std::max(E.h_max_tile, hw.L.max_tile);
        E.h_max_dict = std::max(E.h_max_dict, hw.ndict);
        free_buf(hw.L.d_cid);   // only needed while building
        if (E.bytes > budget) {
            drop_h();
            E.bytes = circuit_bytes;
            break;
        }
    }
    if (!E.h_tables) drop_h();
    // the order in which the workgroups of the <H> kernels take a sweep's tiles: largest first (tile populations are products of
    // binomials, 100 ... 4900 at 24 qubits; numbered order left the longest tiles to the end of a sweep)
    for (SectorHSweep &hw : E.hs) {
        std::vector<uint32_t> hoff((size_t)hw.L.ntiles + 1);
        HIPC(h, hipMemcpyAsync(hoff.data(), hw.L.d_off.p, hoff.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
        HIPC(h, hipStreamSynchronize(h->stream));
        std::vector<uint32_t> ord((size_t)hw.L.ntiles);
        std::iota(ord.begin(), ord.end(), 0u);
        std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return hoff[a + 1] - hoff[a] > hoff[b + 1] - hoff[b]; });
        rc = upload(h, hw.d_torder, ord.data(), ord.size() * sizeof(uint32_t));
        if (rc) return rc;
    }
    std::vector<SecHSweep> desc;
    for (const SectorHSweep &hw : E.hs)
        desc.push_back(SecHSweep{(const uint32_t *)hw.L.d_src.p, (const uint32_t *)hw.L.d_off.p, (const uint16_t *)hw.d_order.p,
                                 (const uint32_t *)hw.d_cbase.p,
                                 (const uint32_t *)hw.d_clen.p, (const uint32_t *)hw.d_cwords.p, (const double *)hw.d_cvals.p,
                                 (const double *)hw.d_dict.p, (const uint32_t *)hw.d_xbase.p, (const uint32_t *)hw.d_xlen.p,
                                 (const uint32_t *)hw.d_xwords.p, (const double *)hw.d_xvals.p, hw.ndict, (int32_t)hw.L.ntiles,
                                 (const uint32_t *)hw.d_torder.p, hw.packed});
    rc = upload(h, E.d_hdesc, desc.data(), desc.size() * sizeof(SecHSweep));
    return rc;
}

// Build the engine for (stored program, stored Hamiltonian).  Leaves E.valid = false (and E.disabled = true) when the program
// does not qualify; errors are returned.  Clobbers the state buffer.
int build_sector_tables_impl(ovqe_handle h, bool allow_regular);
bool sector_reg_fits(const SectorEngine &E);
bool sector_adjoint_reg_fits(ovqe_handle h, const SectorEngine &E);
int build_sector_tables(ovqe_handle h) { return build_sector_tables_impl(h, true); }
int build_sector_tables_impl(ovqe_handle h, bool allow_regular) {
    SectorEngine &E = h->sec;
    const auto t_start = std::chrono::steady_clock::now();
    auto stamp = [&](const char *what) {   // "sector_debug" bit 2 (value 4): wall time of the build's phases on stderr
        if (!(h->opt_sector_debug & 4)) return;
        (void)hipStreamSynchronize(h->stream);
        fprintf(stderr, "ovqe: sector build, %s: %.2f ms since start\n", what,
                1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count());
    };
    free_sector(E);
    E.last_eval_us = 0.0;
    E.disabled = true;   // until everything below succeeded
    E.prog_version = h->prog_version;
    E.ham_version = h->ham.version;
    if (!h->prog_real_ok || h->n_global != 0 || h->n_local > 32 || h->n_local < 8 || !h->ham.set) SEC_DECLINE("program not real-amplitude / sharded / register outside 8..32 qubits / no Hamiltonian");
    // compact ops
    std::vector<SecBuildOp> bops;
    std::vector<SecPat> pats;
    std::vector<int> first_of_sop(h->sops.size() + 1, 0);
    for (size_t o = 0; o < h->sops.size(); ++o) {
        const SmallOp &op = h->sops[o];
        first_of_sop[o] = (int)bops.size();
        if (op.x == 0 || op.x > 0xffffffffull) SEC_DECLINE("an op without x mask or beyond 32 bits");
        if (op.kind == OP_TAB) {
            if (op.count > SEC_MAX_PAT || op.count < 1) SEC_DECLINE("a fused same-x run with more than SEC_MAX_PAT patterns");
            SecBuildOp b = {op.x, h->sop_zc[o], (int32_t)pats.size(), op.count, 0, op.first};
            for (int p = 0; p < op.count; ++p) pats.push_back(SecPat{op.x, h->srots[op.first + p].z});
            bops.push_back(b);
        } else if (op.kind == OP_PAIR) {
            const uint64_t pbit = 1ull << op.pivot;
            const int32_t pat0 = (int32_t)pats.size();
            pats.push_back(SecPat{pbit, 0ull});
            for (int r = 0; r < op.count; ++r) bops.push_back(SecBuildOp{op.x, h->srots[op.first + r].z, pat0, 1, 1, op.first + r});
        } else {
            SEC_DECLINE("an op that is neither a table nor a pair rotation");
        }
    }
    first_of_sop[h->sops.size()] = (int)bops.size();
    if (bops.empty()) SEC_DECLINE("no ops");
    // probe: structural zeros are exact zeros for every theta, and a structurally non-zero amplitude vanishes exactly only
    // on a null set of parameter vectors
    std::vector<double> theta((size_t)std::max(h->K, 1));
    for (int k = 0; k < h->K; ++k) {
        const double f = 0.6180339887498949 * (k + 1);
        theta[k] = 0.4 + 0.7 * (f - std::floor(f));
    }
    stamp("ops listed");
    // the Z2 symmetries of the program (Z-type operators that commute with every rotation string) and the coset through |hf>
    std::vector<int> freebits;
    std::vector<uint64_t> symG;
    uint64_t freemask = 0;
    if (h->opt_sector_regular && allow_regular) {
        std::vector<uint64_t> xs;
        for (const SecBuildOp &b : bops) xs.push_back(b.x);
        z2_symmetries(xs, h->n_local, freebits, symG);
        for (int f : freebits) freemask |= 1ull << f;
    }
    // A GATE LIST in frame form (the reference's QUCCSD templates, which do not conserve the particle number and fill the whole coset)
    // takes the coset AS its support without probing: the dense probe run and the listing of its non-zeros are 40 of the 200 ms to the
    // first energy at 24 qubits.  The coset contains the true support whatever the program does (every x mask maps it to itself), so the
    // tables are exact either way; build_sector checks with one evaluation at generic angles that the coset is populated and comes back
    // here with coset_first off when it is not (a number-conserving gate list: 1/7 of the coset at 24 qubits).
    const int tsym = (int)freebits.size();
    // (at most eight symmetries fit the coset descriptor; a list with more takes the probe path below, as before the coset shortcut)
    const bool coset_first = h->prog_from_gates && !E.coset_rejected && E.probe_mode == 0 && tsym >= 1 && tsym <= 8 &&
                             h->n_local - tsym >= 8 && h->n_local - tsym <= 30 &&
                             (1ull << (h->n_local - tsym)) * (uint64_t)std::max(h->opt_sector_sparsity, 2) <= h->namps;
    E.coset_assumed = coset_first;
    int rc = OVQE_OK;
    uint32_t hf_cid = 0;
    if (coset_first) {
        const uint32_t Kc = 1u << (h->n_local - tsym);
        rc = ensure(h, E.d_sup, (size_t)Kc * sizeof(uint32_t));
        if (rc) return rc;
        SecCoset cz = {};
        cz.kept = (uint32_t)((h->namps - 1ull) & ~freemask);
        cz.nfree = tsym;
        for (int k = 0; k < tsym && k < 8; ++k) {
            cz.fbit[k] = (uint32_t)freebits[k];
            cz.G[k] = (uint32_t)symG[k];
            cz.s[k] = (uint32_t)(((h->hf >> freebits[k]) & 1ull) ^ (uint64_t)(__builtin_popcountll(h->hf & symG[k]) & 1));
        }
        hipLaunchKernelGGL(k_sec_coset, dim3((Kc + 255u) / 256u), dim3(256), 0, h->stream, cz, Kc, (uint32_t *)E.d_sup.p);
        HIPC(h, hipGetLastError());
        E.K = Kc;
        hf_cid = host_pext(h->hf, cz.kept);   // the members ascend with their kept bits: |hf>'s rank is its kept-bit pattern
        stamp("coset listed (no probe)");
    } else {
        h->probe_independent = E.probe_mode == 1;   // second attempt (sector_orphaned): one angle per rotation
        rc = run_program_streaming(h, theta.data(), true);
        if (h->opt_sector_debug & 4)
            fprintf(stderr, "ovqe: sector build, probe launched: %.2f ms since start\n",
                    1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count());
        h->probe_independent = false;
        if (rc) return rc;
        stamp("probe run");
        std::vector<uint32_t> sup;
        rc = sector_support(h, E, sup);
        if (rc) return rc;
        stamp("support listed");
        if (E.K == 0) SEC_DECLINE("the support is empty or more than 1/sector_sparsity of the register");
        const auto hf_it = std::lower_bound(sup.begin(), sup.end(), (uint32_t)h->hf);
        if (hf_it == sup.end() || *hf_it != (uint32_t)h->hf) SEC_DECLINE("the reference determinant is not in the probed support");
        hf_cid = (uint32_t)(hf_it - sup.begin());
    }
    const uint32_t K = E.K;
    // a REGULAR support: the full coset of the program's Z2 symmetries (2^(n - t) amplitudes) — the sweeps then run from bit
    // arithmetic (k_sector_sweep_reg), provided every op has 1..4 kept mixing bits and at most two free bits inside its x mask
    bool regular = false;
    if (h->opt_sector_regular && allow_regular) regular = tsym >= 1 && tsym < h->n_local && (uint64_t)K == (1ull << (h->n_local - tsym));

    SectorScratch W;
    size_t free_b = 0, total_b = 0;
    HIPC(h, hipMemGetInfo(&free_b, &total_b));
    const size_t budget = std::min<size_t>((size_t)std::max(h->opt_sector_max_gb, 0) << 30, free_b / 5 * 3);
    E.budget = budget;
    // slot bits of the pair words: the widest op decides how many bits the pattern field needs
    int maxpat = 1;
    for (const SecBuildOp &b : bops) maxpat = std::max(maxpat, b.npat);
    const int sb_max = maxpat <= 2 ? 15 : (maxpat <= 8 ? 14 : 13);
    const uint32_t tile_cap = std::min<uint32_t>((1u << sb_max) - 2u, (uint32_t)std::max(64, std::min(h->opt_sector_tile_cap, (int)SEC_TILE_LDS_CAP)));
    std::vector<uint32_t> reg_emap;   // regular supports: table-entry map of all sweeps
    // runs of ops without barriers are planned for the workgroup size the sweeps will be launched with (waves own slot sets)
    const int plan_threads = h->opt_sector_reg_threads == 128 || h->opt_sector_reg_threads == 512 || h->opt_sector_reg_threads == 1024
                                 ? h->opt_sector_reg_threads : 256;
    const int plan_wave_bits = h->opt_sector_reg_runs ? __builtin_ctz((unsigned)plan_threads / 64u) : 0;
    E.reg_plan_threads = plan_wave_bits ? plan_threads : 0;
    // a LARGE regular support needs no pair words at all — energies and gradients run from bit arithmetic (the reference's QUCCSD list at
    // 24 qubits: 14 GB of words, 0.16 s of the build) — unless the pair-word kernels are asked for (options, measurements); small ones keep
    // them for the batched evaluations of the second sweep form
    const bool skip_pairs = regular && h->opt_sector_regular == 1 && h->opt_sector_reg_adjoint && K >= (1u << 20);
    for (int M = sector_tile_bits(h); M >= 6; --M) {
        bool too_big = false;
        for (SectorSeg &s : E.segs) {
            free_layout(s.L);
            free_buf(s.d_tab0);
            free_buf(s.d_poff);
            free_buf(s.d_pairs);
            free_buf(s.d_srcpad);
            free_buf(s.d_dstpad);
            free_buf(s.d_wide);
            free_buf(s.d_rounds);
            free_buf(s.d_stream);
            free_buf(s.d_rowhdr);
            free_buf(s.d_rowinfo);
            s.nruns = 0;
            free_buf(s.d_bdst);
        }
        E.segs.clear();
        reg_emap.clear();
        E.npairs = 0;
        E.bytes = 0;
        E.max_tile = 0;
        // ---- circuit: greedy segmentation of the fused program, as build_tile_plan but with no mandatory low bits -------
        size_t o = 0;
        while (o < h->sops.size() && !too_big) {
            uint64_t S = 0;
            size_t j = o;
            while (j < h->sops.size() && __builtin_popcountll(S | h->sops[j].x) <= M) S |= h->sops[j++].x;
            if (j == o) SEC_DECLINE("an op wider than the tile");   // an op wider than the tile
            for (int b = 0; __builtin_popcountll(S) < M; ++b) S |= 1ull << b;
            E.segs.emplace_back();
            SectorSeg &sg = E.segs.back();
            rc = sector_layout(h, E, W, (uint32_t)S, M, sg.L);
            if (rc) return rc;
            if (sg.L.max_tile > tile_cap) {
                too_big = true;
                break;
            }
            if (E.segs.size() == 1) {
                HIPC(h, hipMemcpyAsync(&sg.hf_pos, (const uint32_t *)W.inv.p + hf_cid, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
                HIPC(h, hipStreamSynchronize(h->stream));
            } else {
                rc = sector_compose(h, E, sg.L, W.inv_circ);
                const uint32_t cap = std::max(sg.L.max_tile, 1u);
                if (!rc) rc = ensure(h, sg.d_srcpad, (size_t)sg.L.ntiles * cap * sizeof(uint32_t));
                if (rc) return rc;
                hipLaunchKernelGGL(k_sec_pad_src, dim3(sg.L.ntiles), dim3(256), 0, h->stream, (const uint32_t *)sg.L.d_src.p,
                                   (const uint32_t *)sg.L.d_off.p, cap, (uint32_t *)sg.d_srcpad.p);
                HIPC(h, hipGetLastError());
            }
            // ops of the segment, pattern indices relative to the segment's pattern table
            const int b0 = first_of_sop[o], b1 = first_of_sop[j];
            sg.nops = b1 - b0;
            std::vector<SecBuildOp> sops(bops.begin() + b0, bops.begin() + b1);
            std::vector<SecPat> spats;
            std::vector<int32_t> tab0(sg.nops);
            int rmin = INT32_MAX, rmax = 0;
            for (int k = 0; k < sg.nops; ++k) {
                rmin = std::min(rmin, sops[k].tab0);
                rmax = std::max(rmax, sops[k].tab0 + sops[k].npat);
            }
            sg.rot0 = rmin;
            sg.nrot = rmax - rmin;
            if (sg.nrot > 2048) SEC_DECLINE("more than 2048 rotations in one sweep");   // cos/sin table of a sweep: 32 KB of LDS at most
            for (int k = 0; k < sg.nops; ++k) {
                SecBuildOp &b = sops[k];
                const int32_t p0 = (int32_t)spats.size();
                spats.insert(spats.end(), pats.begin() + b.pat0, pats.begin() + b.pat0 + b.npat);
                b.pat0 = p0;
                tab0[k] = b.tab0;
            }
            const uint32_t nt = sg.L.ntiles;
            if (regular) {   // every tile full, and the sweep's ops in the kernel's shapes
                const int t = (int)freebits.size();
                std::vector<SecRegOp> rops;
                std::vector<uint32_t> emap, gwords;
                std::vector<int> dep;          // this sweep's dependent bits (inside S) and their generators
                std::vector<uint64_t> depG;
                regular = M > t && sg.L.max_tile == (1u << (M - t)) && (uint64_t)sg.L.ntiles * sg.L.max_tile == (uint64_t)K &&
                          sweep_symmetries(freebits, symG, S, h->n_local, dep, depG) &&
                          build_reg_ops(sops, spats, S, (uint64_t)(h->namps - 1ull), h->hf, dep, depG, M - t, h->opt_sector_reg_pairs != 0, rops, emap, gwords,
                                        6, plan_wave_bits, 16);
                if (regular) {
                    uint64_t depmask = 0;
                    for (int f : dep) depmask |= 1ull << f;
                    sg.reg_kept = (uint32_t)(S & ~depmask);
                    sg.nregtab = (int)emap.size();
                    sg.regtab0 = (uint32_t)reg_emap.size();
                    reg_emap.insert(reg_emap.end(), emap.begin(), emap.end());
                    rc = upload(h, sg.d_regops, rops.data(), rops.size() * sizeof(SecRegOp));
                    if (!rc) rc = upload(h, sg.d_reggw, gwords.data(), gwords.size() * sizeof(uint32_t));
                    if (rc) return rc;
                    E.bytes += rops.size() * sizeof(SecRegOp) + emap.size() * (sizeof(uint32_t) + sizeof(double2)) + gwords.size() * sizeof(uint32_t);
                }
            }
            if (skip_pairs && !regular) return build_sector_tables_impl(h, false);   // (a sweep outside the regular kernel's shapes after all)
            if (skip_pairs) {
                sg.npairs = (uint64_t)sg.nops * (K / 2);
                E.npairs += sg.npairs;
                HIPC(h, hipStreamSynchronize(h->stream));
                std::swap(W.inv, W.inv_circ);   // this layout is the next one's source
                E.bytes += (size_t)K * 8;
                E.max_tile = std::max(E.max_tile, sg.L.max_tile);
                if (E.bytes > budget) SEC_DECLINE("circuit tables beyond the budget");
                o = j;
                continue;
            }
            rc = upload(h, W.ops, sops.data(), sops.size() * sizeof(SecBuildOp));
            if (!rc) rc = upload(h, W.pats, spats.data(), spats.size() * sizeof(SecPat));
            if (!rc) rc = upload(h, sg.d_tab0, tab0.data(), tab0.size() * sizeof(int32_t));
            if (!rc) rc = ensure(h, W.cnt, (size_t)nt * sg.nops * sizeof(uint32_t));
            if (rc) return rc;
            constexpr int NTB = 1024;   // (one workgroup per tile: 1024 threads build a tile's pair lists four times as fast as 256 — the table build is part of the time to the first energy)
            const bool dense_map = M <= 16;
            const size_t map_bytes = sec_map_bytes(dense_map, M, sg.L.max_tile, true);
            // second form of the builder (k_sec_pairs2: ops staged in LDS, no barrier per op) whenever its LDS fits; "sector_pairs_form" 1: first form
            const size_t smem2 = sec_pairs2_lds(map_bytes, (int)sops.size(), (int)spats.size(), NTB / 64).bytes;
            const bool form2 = h->opt_sector_pairs_form != 1 && smem2 <= sec_staged_budget(dense_map);
            const size_t smem = form2 ? smem2 : sec_map_bytes(dense_map, M, sg.L.max_tile, false);
            if (form2) {
                rc = ensure(h, W.wbase, (size_t)nt * sg.nops * (NTB / 64) * sizeof(uint32_t));
                if (rc) return rc;
            }
            constexpr size_t PAIRS_LDS_MAX = 144 * 1024;   // (the first form holds the key map alone)
            rc = lds_opt_in<&k_sec_pairs<false, NTB, true>, &k_sec_pairs<true, NTB, true>>(h, PAIRS_LDS_MAX);
            if (!rc) rc = lds_opt_in<&k_sec_pairs2<false, NTB, true>, &k_sec_pairs2<true, NTB, true>>(h, SEC_LDS_MAX);
            if (rc) return rc;
            h->forms_used |= (form2 ? 512u : 256u) | (dense_map ? SECF_PAIRS_DENSE : SECF_PAIRS_SEARCH);
#define OVQE_PAIRS(FILL, DENSE, CNT, POFF, PAIRS)                                                                            \
    do {                                                                                                                    \
        if (form2)                                                                                                          \
            hipLaunchKernelGGL((k_sec_pairs2<FILL, NTB, DENSE>), dim3(nt), dim3(NTB), smem, h->stream, (const uint32_t *)E.d_sup.p, \
                               (const uint32_t *)W.keys.p, (const uint32_t *)sg.L.d_cid.p, (const uint32_t *)sg.L.d_off.p, M, \
                               (uint32_t)S, (const SecBuildOp *)W.ops.p, sg.nops, (const SecPat *)W.pats.p, (int)spats.size(), \
                               (uint32_t)map_bytes, CNT, (uint32_t *)W.wbase.p, POFF, PAIRS, sb_max);                          \
        else                                                                                                                \
            hipLaunchKernelGGL((k_sec_pairs<FILL, NTB, DENSE>), dim3(nt), dim3(NTB), smem, h->stream, (const uint32_t *)E.d_sup.p, \
                               (const uint32_t *)W.keys.p, (const uint32_t *)sg.L.d_cid.p, (const uint32_t *)sg.L.d_off.p, M, \
                               (uint32_t)S, (const SecBuildOp *)W.ops.p, sg.nops, (const SecPat *)W.pats.p, CNT, POFF, PAIRS, sb_max); \
    } while (0)
            if (dense_map) { OVQE_PAIRS(false, true, (uint32_t *)W.cnt.p, (const uint32_t *)nullptr, (uint32_t *)nullptr); }
            else { OVQE_PAIRS(false, false, (uint32_t *)W.cnt.p, (const uint32_t *)nullptr, (uint32_t *)nullptr); }
            HIPC(h, hipGetLastError());
            std::vector<uint32_t> cnt((size_t)nt * sg.nops), poff((size_t)nt * (sg.nops + 1));
            HIPC(h, hipMemcpyAsync(cnt.data(), W.cnt.p, cnt.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
            HIPC(h, hipStreamSynchronize(h->stream));
            uint64_t run = 0;
            for (uint32_t t = 0; t < nt; ++t) {
                for (int k = 0; k < sg.nops; ++k) {
                    poff[(size_t)t * (sg.nops + 1) + k] = (uint32_t)run;
                    run += cnt[(size_t)t * sg.nops + k];
                }
                poff[(size_t)t * (sg.nops + 1) + sg.nops] = (uint32_t)run;
            }
            if (run > 0xfffffff0ull) SEC_DECLINE("pair stream beyond 32-bit offsets");
            sg.max_op_pairs = 0;
            for (uint32_t tt = 0; tt < nt; ++tt)
                for (int oo = 0; oo < sg.nops; ++oo)
                    sg.max_op_pairs = std::max(sg.max_op_pairs, poff[(size_t)tt * (sg.nops + 1) + oo + 1] - poff[(size_t)tt * (sg.nops + 1) + oo]);
            sg.npairs = run;
            E.npairs += run;
            rc = upload(h, sg.d_poff, poff.data(), poff.size() * sizeof(uint32_t));
            if (!rc) rc = ensure(h, sg.d_pairs, (size_t)std::max<uint64_t>(run, 1) * sizeof(uint32_t));
            if (rc) return rc;
            if (dense_map) { OVQE_PAIRS(true, true, (uint32_t *)nullptr, (const uint32_t *)sg.d_poff.p, (uint32_t *)sg.d_pairs.p); }
            else { OVQE_PAIRS(true, false, (uint32_t *)nullptr, (const uint32_t *)sg.d_poff.p, (uint32_t *)sg.d_pairs.p); }
#undef OVQE_PAIRS
            HIPC(h, hipGetLastError());
            // 64-bit words + rounds of the second sweep kernel (single evaluations on large tiles; batches) — for sweeps whose pair
            // stream is latency-bound; a sweep with hundreds of millions of pairs (the reference's QUCCSD templates at 24 qubits:
            // 3.5 G pairs per evaluation) is bound by the bytes of its words, which the 64-bit form doubles: first form there
            if (h->opt_sector_sweep >= 2 && run <= (uint64_t)SEC_WIDE_MAX_PAIRS) {
                uint32_t maxp = 0;
                for (uint32_t tt = 0; tt < nt; ++tt)
                    maxp = std::max(maxp, poff[(size_t)(tt + 1) * (sg.nops + 1) - 1] - poff[(size_t)tt * (sg.nops + 1)]);
                sg.maxchunks = std::max(1u, (maxp + SEC_CHUNK - 1u) / SEC_CHUNK);
                rc = ensure(h, sg.d_wide, (size_t)std::max<uint64_t>(run, 1) * sizeof(uint64_t));
                if (!rc) rc = ensure(h, sg.d_rounds, (size_t)nt * sg.maxchunks * sizeof(uint16_t));
                if (rc) return rc;
                hipLaunchKernelGGL(k_sec_widen, dim3(nt), dim3(256), 0, h->stream, (const uint32_t *)sg.d_pairs.p, (const uint32_t *)sg.d_poff.p,
                                   (const int32_t *)sg.d_tab0.p, sg.nops, sg.rot0, sb_max, sg.maxchunks, SEC_CHUNK, (uint64_t *)sg.d_wide.p,
                                   (uint16_t *)sg.d_rounds.p);
                HIPC(h, hipGetLastError());
                E.bytes += (size_t)run * 8 + (size_t)nt * sg.maxchunks * 2;
                if (h->opt_sector_sweep >= 3) {
                    rc = build_wave_streams(h, E, W, sg, sops, maxp, S, M, sb_max);
                    if (rc) return rc;
                }
            }
            HIPC(h, hipStreamSynchronize(h->stream));
            std::swap(W.inv, W.inv_circ);   // this layout is the next one's source
            E.bytes += (size_t)K * 8 + poff.size() * 4 + (size_t)run * 4;
            E.max_tile = std::max(E.max_tile, sg.L.max_tile);
            if (E.bytes > budget) SEC_DECLINE("circuit tables beyond the budget");
            o = j;
        }
        if (too_big) continue;
        E.M = M;
        E.sb = sb_max;
        break;
    }
    E.regular = regular && !E.segs.empty();
    E.freemask = (uint32_t)freemask;
    E.reg_m = E.M - (int)freebits.size();
    for (const SectorSeg &sg : E.segs) E.regular = E.regular && sg.d_regops.p != nullptr;
    if (E.regular && E.reg_m <= 16 && h->opt_sector_regular != 3) {
        // gathers in runs: sweep s stores slot k of a tile at position pos_s[k] — the kept bits it shares with sweep s + 1 lowest —
        // and sweep s + 1 walks its gather in the same order (3: canonical order everywhere, measurements)
        const uint32_t cap = 1u << E.reg_m;
        auto slot_perm = [&](uint32_t kept, uint32_t shared, std::vector<uint16_t> &slot_of_pos) {
            // position j -> slot: position bits = (shared kept bits ascending, then the other kept bits ascending)
            std::vector<int> bits, sh, rest;
            for (int p = 0; p < 32; ++p)
                if ((kept >> p) & 1u) {
                    bits.push_back(p);
                    (((shared >> p) & 1u) ? sh : rest).push_back(p);
                }
            sh.insert(sh.end(), rest.begin(), rest.end());
            std::vector<int> slotbit(32, 0);
            for (size_t q = 0; q < bits.size(); ++q) slotbit[bits[q]] = (int)q;
            slot_of_pos.assign(cap, 0);
            for (uint32_t j = 0; j < cap; ++j) {
                uint32_t k = 0;
                for (size_t q = 0; q < sh.size(); ++q) k |= ((j >> q) & 1u) << slotbit[sh[q]];
                slot_of_pos[j] = (uint16_t)k;
            }
        };
        DevBuf d_pos;
        for (size_t si = 0; si + 1 < E.segs.size() && !rc; ++si) {
            SectorSeg &a = E.segs[si], &b = E.segs[si + 1];
            const uint32_t shared = a.reg_kept & b.reg_kept;
            std::vector<uint16_t> oslot, gslot, pos(cap);
            slot_perm(a.reg_kept, shared, oslot);
            slot_perm(b.reg_kept, shared, gslot);
            for (uint32_t j = 0; j < cap; ++j) pos[oslot[j]] = (uint16_t)j;
            rc = upload(h, a.d_regoslot, oslot.data(), cap * sizeof(uint16_t));
            if (!rc) rc = upload(h, b.d_reggslot, gslot.data(), cap * sizeof(uint16_t));
            if (!rc) rc = upload(h, d_pos, pos.data(), cap * sizeof(uint16_t));
            if (!rc) rc = ensure(h, b.d_regsrc, (size_t)b.L.ntiles * cap * sizeof(uint32_t));
            if (rc) break;
            hipLaunchKernelGGL(k_sec_reg_src, dim3(b.L.ntiles), dim3(256), 0, h->stream, (const uint32_t *)b.d_srcpad.p,
                               (const uint16_t *)b.d_reggslot.p, (const uint16_t *)d_pos.p, cap, (uint32_t *)b.d_regsrc.p);
            if (hipStreamSynchronize(h->stream) != hipSuccess) rc = fail(h, OVQE_ERR_HIP, "sector: gather tables of the regular sweeps");
            E.bytes += (size_t)b.L.ntiles * cap * sizeof(uint32_t) + 2 * cap * sizeof(uint16_t);
        }
        free_buf(d_pos);
        if (rc) return rc;
    }
    if (skip_pairs && !(E.regular && sector_reg_fits(E) && sector_adjoint_reg_fits(h, E)))
        return build_sector_tables_impl(h, false);   // the kernels that do without pair words cannot take this engine after all
    if (E.regular) {
        E.nregtab = (uint32_t)reg_emap.size();
        rc = upload(h, E.d_regmap, reg_emap.data(), std::max<size_t>(reg_emap.size(), 1) * sizeof(uint32_t));
        if (!rc) rc = ensure(h, E.d_regtab, std::max<size_t>(reg_emap.size(), 1) * sizeof(double2));
        if (rc) return rc;
    }
    if (E.segs.empty() || E.M == 0) SEC_DECLINE("no tile size fits (largest tile above sector_tile_cap for every M)");
    {   // the second form needs its tables for EVERY sweep
        bool all_wide = true;
        for (const SectorSeg &sg : E.segs) all_wide = all_wide && sg.d_wide.p != nullptr;
        if (!all_wide)
            for (SectorSeg &sg : E.segs) {
                if (sg.d_wide.p) E.bytes -= std::min(E.bytes, (size_t)sg.npairs * 8 + (size_t)sg.L.ntiles * sg.maxchunks * 2);
                free_buf(sg.d_wide);
                free_buf(sg.d_rounds);
                free_buf(sg.d_stream);
                free_buf(sg.d_rowhdr);
                free_buf(sg.d_rowinfo);
                sg.nruns = 0;
            }
    }
    stamp("circuit tables");
    // scatter tables of the second sweep kernel: every sweep writes its tile straight into the next sweep's tile-padded order
    if (!E.segs.empty() && E.segs[0].d_wide.p) {
        DevBuf dstc;
        size_t pad = 0;
        bool fits = true;
        for (const SectorSeg &sg : E.segs) {
            const size_t e = (size_t)sg.L.ntiles * std::max(sg.L.max_tile, 1u);
            pad = std::max(pad, e);
            fits = fits && e < 0xffffffffull;
        }
        rc = fits ? ensure(h, dstc, (size_t)K * sizeof(uint32_t)) : OVQE_OK;
        for (size_t si = 0; fits && !rc && si < E.segs.size(); ++si) {
            SectorSeg &sg = E.segs[si];
            const uint32_t cap = std::max(sg.L.max_tile, 1u);
            rc = ensure(h, sg.d_dstpad, (size_t)sg.L.ntiles * cap * sizeof(uint32_t));
            if (rc) break;
            const bool last = si + 1 == E.segs.size();
            if (!last) {
                const SectorSeg &nx = E.segs[si + 1];
                hipLaunchKernelGGL(k_sec_dst_compact, dim3(nx.L.ntiles), dim3(256), 0, h->stream, (const uint32_t *)nx.L.d_src.p,
                                   (const uint32_t *)nx.L.d_off.p, std::max(nx.L.max_tile, 1u), (uint32_t *)dstc.p);
            }
            hipLaunchKernelGGL(k_sec_dst_pad, dim3(sg.L.ntiles), dim3(256), 0, h->stream, last ? (const uint32_t *)nullptr : (const uint32_t *)dstc.p,
                               (const uint32_t *)sg.L.d_off.p, cap, (uint32_t *)sg.d_dstpad.p);
            E.bytes += (size_t)sg.L.ntiles * cap * sizeof(uint32_t);
        }
        // sweeps with several tiles per CU take them largest first (k_sector_sweep2's torder)
        for (size_t si = 0; fits && !rc && si < E.segs.size(); ++si) {
            SectorSeg &sg = E.segs[si];
            if (sg.L.ntiles < 512u) continue;
            std::vector<uint32_t> hoff((size_t)sg.L.ntiles + 1), ord((size_t)sg.L.ntiles);
            if (hipMemcpyAsync(hoff.data(), sg.L.d_off.p, hoff.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
                hipStreamSynchronize(h->stream) != hipSuccess) {
                rc = fail(h, OVQE_ERR_HIP, "sector: tile order");
                break;
            }
            std::iota(ord.begin(), ord.end(), 0u);
            std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return hoff[a + 1] - hoff[a] > hoff[b + 1] - hoff[b]; });
            rc = upload(h, sg.d_torder, ord.data(), ord.size() * sizeof(uint32_t));
        }
        // ... and the backward sweeps of the gradient into the PREVIOUS sweep's (k_sector_adjoint2)
        for (size_t si = 1; fits && !rc && si < E.segs.size(); ++si) {
            SectorSeg &sg = E.segs[si];
            const SectorSeg &pv = E.segs[si - 1];
            const uint32_t cap = std::max(sg.L.max_tile, 1u);
            rc = ensure(h, sg.d_bdst, (size_t)sg.L.ntiles * cap * sizeof(uint32_t));
            if (rc) break;
            hipLaunchKernelGGL(k_sec_padpos, dim3(pv.L.ntiles), dim3(256), 0, h->stream, (const uint32_t *)pv.L.d_off.p,
                               std::max(pv.L.max_tile, 1u), (uint32_t *)dstc.p);
            hipLaunchKernelGGL(k_sec_bdst, dim3(sg.L.ntiles), dim3(256), 0, h->stream, (const uint32_t *)sg.L.d_src.p,
                               (const uint32_t *)sg.L.d_off.p, cap, (const uint32_t *)dstc.p, (uint32_t *)sg.d_bdst.p);
            E.bytes += (size_t)sg.L.ntiles * cap * sizeof(uint32_t);
        }
        if (!rc && hipGetLastError() != hipSuccess) rc = fail(h, OVQE_ERR_HIP, "sector: dst tables");
        if (!rc && hipStreamSynchronize(h->stream) != hipSuccess) rc = fail(h, OVQE_ERR_HIP, "sector: dst tables (sync)");
        free_buf(dstc);
        if (rc) return rc;
        E.pad_elems = fits ? pad : 0;
    }
    // position of the reference determinant in the circuit's final order (ovqe_sector_ground_state starts from its block)
    HIPC(h, hipMemcpyAsync(&E.hf_final, (const uint32_t *)W.inv_circ.p + hf_cid, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));

    stamp("scatter tables");
    rc = build_sector_h(h, E, W, budget);
    stamp("<H> tables");
    if (!rc) rc = ensure(h, E.d_buf[0], std::max<size_t>(K, E.pad_elems) * sizeof(double));
    if (!rc) rc = ensure(h, E.d_buf[1], std::max<size_t>(K, E.pad_elems) * sizeof(double));
    if (!rc) rc = ensure(h, E.d_flag, 256);
    if (rc) return rc;
    HIPC(h, hipMemsetAsync(E.d_flag.p, 0, sizeof(int), h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    for (size_t s = 0; s + 1 < E.segs.size(); ++s) free_buf(E.segs[s].L.d_cid);   // the last one maps the result to canonical order
    if (h->opt_sector_debug & 2)
        fprintf(stderr, "ovqe: sector tables built: support %u, %zu circuit sweeps (tile bits %d, largest tile %u), %zu <H> sweeps (tile bits %d, largest tile %u, "
                        "largest dictionary %d), %.2f GB\n", E.K, E.segs.size(), E.M, E.max_tile, E.hs.size(), E.Mh, E.h_max_tile, E.h_max_dict, 1e-9 * (double)E.bytes);
    E.valid = true;
    E.disabled = false;
    return OVQE_OK;
}

int run_sector_circuit(ovqe_handle h, const double *theta, int *last);
int build_sector(ovqe_handle h) {
    // the previous engine's blocks go back to the driver BEFORE the build's block cache opens: kept, they would sit in the cache
    // while the budget is taken from hipMemGetInfo (old + new tables resident at once, a budget smaller by the old tables' size)
    free_sector_kept(h, h->sec);
    DevBlockScope kept_blocks(h->kept_blocks);
    int rc = build_sector_tables(h);
    SectorEngine &E = h->sec;
    if (!rc && E.valid && E.coset_assumed) {
        // the coset was taken as the support without a probe (a gate list): one evaluation of the circuit at generic angles on the new
        // tables, and a count of what it populates.  Less than half: the program keeps more symmetries than the Z2 ones (a particle
        // number, say) — the tables would be exact but several times larger than needed; rebuilt from a probe.
        std::vector<double> theta((size_t)std::max(h->K, 1));
        for (int k = 0; k < h->K; ++k) {
            const double f = 0.6180339887498949 * (k + 1);
            theta[k] = 0.4 + 0.7 * (f - std::floor(f));
        }
        int last = 0;
        rc = run_sector_circuit(h, theta.data(), &last);
        uint64_t nz = 0;
        if (!rc) {
            const uint64_t per_block = 256ull * SEC_NZ_PER_THREAD;
            const unsigned nb = (unsigned)(((uint64_t)E.K + per_block - 1) / per_block);
            DevBuf d_cnt;
            rc = ensure(h, d_cnt, (size_t)nb * sizeof(uint32_t));
            if (!rc) {
                hipLaunchKernelGGL(k_sec_count_nz, dim3(nb), dim3(256), 0, h->stream, (const double *)E.d_buf[last].p, (uint64_t)E.K,
                                   (uint32_t *)d_cnt.p);
                std::vector<uint32_t> cnt(nb);
                if (hipMemcpyAsync(cnt.data(), d_cnt.p, (size_t)nb * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
                    hipStreamSynchronize(h->stream) != hipSuccess)
                    rc = fail(h, OVQE_ERR_HIP, "sector: census of the coset");
                for (uint32_t c : cnt) nz += c;
            }
            free_buf(d_cnt);
        }
        if (!rc && nz * 2 < (uint64_t)E.K) {
            if (h->opt_sector_debug & 2)
                fprintf(stderr, "ovqe: the program populates %llu of the coset's %u amplitudes: tables rebuilt from a probe\n", (unsigned long long)nz, E.K);
            free_sector(E);
            E.coset_rejected = true;
            rc = build_sector_tables(h);
        }
    }
    if (rc == OVQE_ERR_ALLOC) {   // the device is short of memory (other handles, other processes): the dense kernels serve
        (void)hipGetLastError();
        E.valid = false;
        rc = OVQE_OK;
    }
    if (!E.valid) {   // not eligible (or failed): nothing is kept but the verdict
        const int pv = E.prog_version, hv = E.ham_version;
        free_sector(E);
        E.disabled = true;
        E.prog_version = pv;
        E.ham_version = hv;
    }
    return rc;
}

template <int NT>
int launch_sector_sweeps(ovqe_handle h, SectorEngine &E, int *last) {
    if (int rc = lds_opt_in<&k_sector_sweep<NT>, &k_sector_sweep<NT, true>>(h, LDS_WG_MAX)) return rc;
    int cur = 0;
    for (size_t s = 0; s < E.segs.size(); ++s) {
        const SectorSeg &sg = E.segs[s];
        const uint32_t cap = std::max(sg.L.max_tile, 1u);
        const size_t smem = sec_sweep_lds(cap, sg.nrot, sg.nops).bytes;
        // two chunks of pair words ahead where every op of a tile fits a staging buffer
        const bool d2 = NT > 64 && sg.max_op_pairs <= SEC_STAGE_WORDS && !(h->opt_sector_debug & 1);
        h->forms_used |= 1u | (d2 ? SECF_SWEEP1_AHEAD : SECF_SWEEP1_PLAIN) | secf_wg(SECF_WG_SWEEP, NT);
        if (d2)
            hipLaunchKernelGGL((k_sector_sweep<NT, true>), dim3(sg.L.ntiles), dim3(NT), smem, h->stream, (const double *)E.d_buf[cur ^ 1].p,
                               (double *)E.d_buf[cur].p, s ? (const uint32_t *)sg.d_srcpad.p : (const uint32_t *)nullptr,
                               (const uint32_t *)sg.L.d_off.p, (const int32_t *)sg.d_tab0.p, sg.nops, (const uint32_t *)sg.d_poff.p,
                               (const uint32_t *)sg.d_pairs.p, (const RotParam *)h->d_rp.p, sg.rot0, sg.nrot, cap, sg.hf_pos,
                               (int *)E.d_flag.p, 0, E.sb);
        else
        hipLaunchKernelGGL((k_sector_sweep<NT>), dim3(sg.L.ntiles), dim3(NT), smem, h->stream, (const double *)E.d_buf[cur ^ 1].p,
                           (double *)E.d_buf[cur].p, s ? (const uint32_t *)sg.d_srcpad.p : (const uint32_t *)nullptr,
                           (const uint32_t *)sg.L.d_off.p, (const int32_t *)sg.d_tab0.p, sg.nops, (const uint32_t *)sg.d_poff.p,
                           (const uint32_t *)sg.d_pairs.p, (const RotParam *)h->d_rp.p, sg.rot0, sg.nrot, cap, sg.hf_pos,
                           (int *)E.d_flag.p, h->opt_sector_debug & 1, E.sb);
        *last = cur;
        cur ^= 1;
    }
    HIPC(h, hipGetLastError());
    return OVQE_OK;
}

// second form: scatter-on-write between tile-padded orders, 64-bit pair words in registers (k_sector_sweep2)
template <int NT, int WPT>
int launch_sector_sweeps2(ovqe_handle h, SectorEngine &E, double *buf0, double *buf1, size_t stride, const RotParam *rp, size_t rp_stride,
                          int B, int *last, bool dst_lds) {
    if (int rc = lds_opt_in<&k_sector_sweep2<NT, WPT>>(h, LDS_WG_MAX)) return rc;
    double *buf[2] = {buf0, buf1};
    int cur = 0;
    for (size_t s = 0; s < E.segs.size(); ++s) {
        const SectorSeg &sg = E.segs[s];
        const uint32_t cap = std::max(sg.L.max_tile, 1u);
        const size_t smem = sec_sweep2_lds(cap, sg.nrot, dst_lds, sg.maxchunks).bytes;
        if (smem > LDS_WG_MAX || sg.maxchunks > (uint32_t)NT) return fail(h, OVQE_ERR_INVALID, "internal: sector tile exceeds LDS");
        const bool bfast = B > 1 && sg.L.ntiles <= 65535u;
        if constexpr (NT == 64 * SEC_STREAM_WAVES) {
            const size_t smem3 = sec_sweep2_lds(cap, sg.nrot, dst_lds, 0).bytes;   // (no round counts)
            // third form: per-wave streams, barriers at the run boundaries — for ONE state: the workgroups of a batch hide each other's barriers, and the
            // streams gain them nothing (24 qubits, per evaluation: batches of 64 0.509 ms on the second form / 0.512 on the streams, of 8 0.649 / 0.656)
            if (sg.nruns > 0 && h->opt_sector_sweep >= 3 && smem3 <= LDS_WG_MAX && (B == 1 || h->opt_sector_sweep >= 4)) {
                if (int rc = lds_opt_in<&k_sector_sweep3<NT>>(h, LDS_WG_MAX)) return rc;
                h->forms_used |= 4u | (dst_lds ? SECF_DST_LDS : SECF_DST_LATE) | secf_wg(SECF_WG_SWEEP, NT);
                hipLaunchKernelGGL((k_sector_sweep3<NT>), bfast ? dim3((unsigned)B, sg.L.ntiles) : dim3(sg.L.ntiles, (unsigned)B), dim3(NT),
                                   smem3, h->stream,
                                   s ? (const double *)buf[cur ^ 1] : (const double *)nullptr, buf[cur], stride, stride,
                                   (const uint32_t *)sg.d_dstpad.p, (const uint32_t *)sg.L.d_off.p, (const uint32_t *)sg.d_rowinfo.p, sg.nruns, sg.stream_waves,
                                   (const uint32_t *)sg.d_stream.p, (const uint16_t *)sg.d_rowhdr.p, rp, rp_stride, sg.rot0, sg.nrot, cap,
                                   sg.hf_pos, (int *)E.d_flag.p, E.sb, dst_lds ? 1 : 0, bfast ? 1 : 0, (const uint32_t *)sg.d_torder.p,
                                   h->opt_sector_sweep_dbg & 15);
                *last = cur;
                cur ^= 1;
                continue;
            }
        }
        h->forms_used |= 2u | (dst_lds ? SECF_DST_LDS : SECF_DST_LATE) | secf_wg(SECF_WG_SWEEP, NT);
        for (int rep = 0; rep < (h->opt_sector_sweep_dbg == 16 ? 2 : 1); ++rep)   // 16: every sweep twice (idempotent): cold against warm
        hipLaunchKernelGGL((k_sector_sweep2<NT, WPT>), bfast ? dim3((unsigned)B, sg.L.ntiles) : dim3(sg.L.ntiles, (unsigned)B), dim3(NT), smem, h->stream,
                           s ? (const double *)buf[cur ^ 1] : (const double *)nullptr, buf[cur], stride, stride,
                           (const uint32_t *)sg.d_dstpad.p, (const uint32_t *)sg.L.d_off.p, (const uint32_t *)sg.d_poff.p, sg.nops,
                           (const uint64_t *)sg.d_wide.p, (const uint16_t *)sg.d_rounds.p, sg.maxchunks, rp, rp_stride, sg.rot0, sg.nrot,
                           cap, sg.hf_pos, (int *)E.d_flag.p, (h->opt_sector_sweep_dbg & 15) ? (h->opt_sector_sweep_dbg & 15) : (h->opt_sector_debug & 1),
                           dst_lds ? 1 : 0, bfast ? 1 : 0, (const uint32_t *)sg.d_torder.p);
        *last = cur;
        cur ^= 1;
    }
    HIPC(h, hipGetLastError());
    return OVQE_OK;
}
// B states: buf[i] holds B slices of `stride` doubles, rp B tables of rp_stride entries; the result of every state is left
// contiguous (K doubles at b * stride) in buf[*last]
int sector_sweeps2(ovqe_handle h, SectorEngine &E, int nt, double *buf0, double *buf1, size_t stride, const RotParam *rp, size_t rp_stride,
                   int B, int *last, bool dst_lds = true) {
    switch (nt) {   // words per thread: SEC_CHUNK / threads
    case 1024: return launch_sector_sweeps2<1024, SEC_CHUNK / 1024>(h, E, buf0, buf1, stride, rp, rp_stride, B, last, dst_lds);
    case 512: return launch_sector_sweeps2<512, SEC_CHUNK / 512>(h, E, buf0, buf1, stride, rp, rp_stride, B, last, dst_lds);
    case 256: return launch_sector_sweeps2<256, SEC_CHUNK / 256>(h, E, buf0, buf1, stride, rp, rp_stride, B, last, dst_lds);
    }
    return fail(h, OVQE_ERR_INVALID, "no second sweep form for this workgroup size");
}

// whether the second form has an instantiation for this workgroup size and every tile of the engine fits its LDS: checked
// BEFORE the first launch, so that a caller can take the first form (or the one-at-a-time path) instead of failing half way
bool sector_sweeps2_fits(const SectorEngine &E, int nt, bool dst_lds) {
    if (nt != 1024 && nt != 512 && nt != 256) return false;
    for (const SectorSeg &sg : E.segs) {
        const uint32_t cap = std::max(sg.L.max_tile, 1u);
        if (sec_sweep2_lds(cap, sg.nrot, dst_lds, sg.maxchunks).bytes > LDS_WG_MAX || sg.maxchunks > (uint32_t)nt) return false;
    }
    return true;
}

// launch geometry of the <H> kernels: workgroups per sweep (their dynamic LDS: sec_h_lds_bytes / sec_expect_lds_bytes, sv_sector.hpp)
constexpr int SEC_H_THREADS = 512;
constexpr uint32_t SEC_H_GROUPS = 256;   // workgroups per <H> sweep (they share the sweep's tiles round robin)
uint32_t sector_h_groups(const SectorEngine &E) { return std::min<uint32_t>(E.hs[0].L.ntiles, SEC_H_GROUPS); }

// sweeps of a regular support (k_sector_sweep_reg): no pair words, every tile 2^reg_m slots
template <int NT>
int launch_sector_sweeps_reg(ovqe_handle h, SectorEngine &E, int *last) {
    if (int rc = lds_opt_in<&k_sector_sweep_reg<NT>>(h, LDS_WG_MAX)) return rc;
    hipLaunchKernelGGL(k_sec_reg_angles, dim3((E.nregtab + 255u) / 256u), dim3(256), 0, h->stream, (const uint32_t *)E.d_regmap.p, E.nregtab,
                       (const RotParam *)h->d_rp.p, (double2 *)E.d_regtab.p);
    int cur = 0;
    for (size_t s = 0; s < E.segs.size(); ++s) {
        const SectorSeg &sg = E.segs[s];
        const size_t smem = sec_reg_lds(E.reg_m, 1, sg.nops, 0, 0).bytes;
        h->forms_used |= 8u | secf_wg(SECF_WG_REGULAR, NT);
        hipLaunchKernelGGL((k_sector_sweep_reg<NT>), dim3(sg.L.ntiles), dim3(NT), smem, h->stream, (const double *)E.d_buf[cur ^ 1].p,
                           (double *)E.d_buf[cur].p,
                           s ? (const uint32_t *)(sg.d_regsrc.p ? sg.d_regsrc.p : sg.d_srcpad.p) : (const uint32_t *)nullptr,
                           (const SecRegOp *)sg.d_regops.p, h->opt_sector_sweep_dbg == 1 ? 0 : sg.nops, (const uint32_t *)sg.d_reggw.p,
                           (const double2 *)E.d_regtab.p + sg.regtab0, E.reg_m, sg.hf_pos, h->opt_sector_sweep_dbg,
                           (const uint16_t *)sg.d_reggslot.p, (const uint16_t *)sg.d_regoslot.p,
                           (E.reg_plan_threads == NT && h->opt_sector_reg_runs) ? 0 : 1);
        *last = cur;
        cur ^= 1;
    }
    HIPC(h, hipGetLastError());
    return OVQE_OK;
}
bool sector_reg_fits(const SectorEngine &E) {
    if (!E.regular || E.segs.empty()) return false;
    for (const SectorSeg &sg : E.segs)
        if (!sg.d_regops.p || sec_reg_lds(E.reg_m, 1, sg.nops, 0, 0).bytes > LDS_WG_MAX) return false;
    return true;
}

// The circuit on the sector tables: the compact state in the order of the last sweep is left in E.d_buf[*last].
int run_sector_circuit(ovqe_handle h, const double *theta, int *last) {
    SectorEngine &E = h->sec;
    int rc = resolve_angles(h, theta, true);
    if (rc) return rc;
    if (h->opt_sector_regular && sector_reg_fits(E)) {
        switch (h->opt_sector_reg_threads) {
        case 128: return launch_sector_sweeps_reg<128>(h, E, last);
        case 512: return launch_sector_sweeps_reg<512>(h, E, last);
        case 1024: return launch_sector_sweeps_reg<1024>(h, E, last);
        default: return launch_sector_sweeps_reg<256>(h, E, last);
        }
    }
    if (!E.segs.empty() && !E.segs[0].d_pairs.p) return fail(h, OVQE_ERR_STATE, "internal: sector engine without pair words outside the regular sweeps");
    int nt = h->opt_sector_threads;
    if (nt == 0) {   // automatic: enough threads for one pass over the pairs of an op in an average tile
        const double avg = (double)E.K / (double)std::max<uint64_t>(1, h->namps >> E.M);
        nt = avg >= 1500.0 ? 1024 : (avg >= 600.0 ? 512 : 256);
    }
    // second form whenever its tables exist, one 1024-thread workgroup per tile unless another size is asked for (measured, ms per
    // evaluation, first form at its own best size against this: 18 qubits 0.54 / 0.55, 20 qubits 0.59 / 0.50, 22 qubits 0.91 / 0.85,
    // 24 qubits 1.78 / 1.57, 26 qubits 7.25 / 6.78)
    if (h->opt_sector_sweep >= 2 && E.pad_elems && E.segs[0].d_wide.p && h->opt_sector_threads != 64) {
        // three or more tiles per CU (26 qubits and beyond): what a batch gains from co-resident workgroups a single state gains
        // too — 512-thread workgroups that read their scatter indices at the end, three per CU instead of two of 1024 threads
        const bool many = E.segs[0].L.ntiles >= 768u;
        const int nt2 = h->opt_sector_threads != 0 ? nt : (many ? 512 : 1024);
        if (sector_sweeps2_fits(E, nt2, !(many && h->opt_sector_threads == 0)))   // else: the first form below serves every geometry
        return sector_sweeps2(h, E, nt2, (double *)E.d_buf[0].p, (double *)E.d_buf[1].p, std::max<size_t>(E.K, E.pad_elems),
                              (const RotParam *)h->d_rp.p, 0, 1, last, !(many && h->opt_sector_threads == 0));
    }
    switch (nt) {
    case 64: return launch_sector_sweeps<64>(h, E, last);
    case 512: return launch_sector_sweeps<512>(h, E, last);
    case 1024: return launch_sector_sweeps<1024>(h, E, last);
    default: return launch_sector_sweeps<256>(h, E, last);
    }
}

// ... and in canonical (ascending index) order in psic; *ok = false as below
int run_sector_state(ovqe_handle h, const double *theta, double *psic, bool *ok) {
    SectorEngine &E = h->sec;
    *ok = false;
    int last = 0;
    int rc = run_sector_circuit(h, theta, &last);
    if (rc) return rc;
    hipLaunchKernelGGL(k_sec_scatter, dim3((E.K + 255u) / 256u), dim3(256), 0, h->stream, (const double *)E.d_buf[last].p,
                       (const uint32_t *)E.segs.back().L.d_cid.p, E.K, psic);
    HIPC(h, hipGetLastError());
    HIPC(h, hipMemcpyAsync(h->h_result + 1, E.d_flag.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    int flag = 0;
    std::memcpy(&flag, h->h_result + 1, sizeof(int));
    *ok = flag == 0;
    return OVQE_OK;
}

// mapped host buffer the final reduction of a lone evaluation writes to (k_sector_finish)
bool sector_fin_ready(ovqe_handle h) {
    if (h->h_fin) return true;
    if (h->fin_failed) return false;
    h->fin_failed = true;   // until everything below succeeded
    if (!h->h_fin) {
        if (hipHostMalloc((void **)&h->h_fin, 8 * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) {
            h->h_fin = nullptr;
            (void)hipGetLastError();
            return false;
        }
        if (hipHostGetDevicePointer((void **)&h->d_fin, h->h_fin, 0) != hipSuccess) {
            (void)hipHostFree(h->h_fin);
            h->h_fin = nullptr;
            (void)hipGetLastError();
            return false;
        }
    }
    h->fin_failed = false;
    return true;
}

// E(theta) on the sector tables; *ok = false when a structurally-zero amplitude turned up non-zero (the tables do not
// describe this program: the caller falls back to the dense kernels and disables the engine)
int run_sector_energy(ovqe_handle h, const double *theta, double2 *out, bool *ok) {
    SectorEngine &E = h->sec;
    *ok = false;
    const bool profile = h->opt_sector_profile != 0;
    if (profile) {
        for (hipEvent_t &e : E.ev)
            if (!e) HIPC(h, hipEventCreate(&e));
        HIPC(h, hipEventRecord(E.ev[0], h->stream));
    }
    int last = 0;
    int rc = run_sector_circuit(h, theta, &last);
    if (rc) return rc;
    if (profile) HIPC(h, hipEventRecord(E.ev[1], h->stream));
    const uint32_t nt = sector_h_groups(E);
    const size_t nparts = (size_t)nt * E.hs.size();
    rc = ensure(h, h->d_partials, nparts * sizeof(double2));
    if (!rc) rc = ensure(h, h->d_result, 64 * sizeof(double2));
    if (!rc) rc = lds_opt_in<&k_sector_expect<SEC_H_THREADS>>(h, SEC_LDS_MAX);
    if (rc) return rc;
    // "sector_fused_reduce" (default): the reduction writes energy + flag into mapped host memory (no copies behind it)
    const bool fused = h->opt_sector_fused_reduce && sector_fin_ready(h);
    hipLaunchKernelGGL((k_sector_expect<SEC_H_THREADS>), dim3(nt, (unsigned)E.hs.size()), dim3(SEC_H_THREADS),
                       sec_expect_lds_bytes(std::max(E.h_max_tile, 1u), (uint32_t)E.h_max_dict),
                       h->stream, (const double *)E.d_buf[last].p, (const SecHSweep *)E.d_hdesc.p, (double2 *)h->d_partials.p,
                       std::max(E.h_max_tile, 1u), h->opt_sector_h_dbg);
    if (profile) HIPC(h, hipEventRecord(E.ev[2], h->stream));
    // (polling only where the previous evaluation of these tables took less than 2 ms: a spinning core is the wrong way to wait longer)
    const bool poll = fused && h->opt_poll_result && !profile && E.last_eval_us > 0.0 && E.last_eval_us < 2000.0;
    const auto t_eval = std::chrono::steady_clock::now();
    if (fused) {
        if (poll) std::memcpy(h->h_fin + 3, &OVQE_POLL_SENTINEL, sizeof(uint64_t));
        hipLaunchKernelGGL(k_sector_finish, dim3(1), dim3(256), 0, h->stream, (const double2 *)h->d_partials.p, (int64_t)nparts,
                           (const int *)E.d_flag.p, h->d_fin);
    } else {
        if ((rc = enqueue_reduce(h, h->d_partials.p, (int64_t)nparts))) return rc;
        HIPC(h, hipMemcpyAsync(h->h_result, h->d_result.p, sizeof(double2), hipMemcpyDeviceToHost, h->stream));
        HIPC(h, hipMemcpyAsync(h->h_result + 1, E.d_flag.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    }
    HIPC(h, hipGetLastError());
    if (!poll || !poll_mapped_slot(reinterpret_cast<volatile uint64_t *>(h->h_fin + 3))) HIPC(h, hipStreamSynchronize(h->stream));
    E.last_eval_us = 1e6 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t_eval).count();   // <H> launch to result
    if (profile) {
        HIPC(h, hipEventElapsedTime(&E.last_circuit_ms, E.ev[0], E.ev[1]));
        HIPC(h, hipEventElapsedTime(&E.last_expect_ms, E.ev[1], E.ev[2]));
    }
    int flag = 0;
    if (fused) {
        h->h_result[0] = make_double2(h->h_fin[0], h->h_fin[1]);
        flag = (int)h->h_fin[2];
    } else {
        std::memcpy(&flag, h->h_result + 1, sizeof(int));
    }
    if (flag) {
        if (h->opt_sector_debug & 2) fprintf(stderr, "ovqe: sector tables dropped: an amplitude outside the probed support became non-zero (flag %d)\n", flag);
        return OVQE_OK;
    }
    *out = h->h_result[0];
    *ok = true;
    return OVQE_OK;
}

int sector_matvec(ovqe_handle h, SectorEngine &E, const double *in, double *out);

// B evaluations on the sector tables in one pass each of the circuit's pair words and of the materialised <H>
// (ref:openvqe/ucc_family/get_energy_ucc.py:158-175: scipy's BFGS with jac=None evaluates K + 1 points per gradient;
// `batched_gradient` of the mirrors submits them as one batch): the sweeps run with blockIdx.y = state (own tile-padded
// slices and angle tables), <H> holds NB = 2 states per tile so the table streams once per pair of states.
// theta: B x K on the host or (theta_on_device) on the device; energies likewise.  *ok = false: an orphan pair was hit by
// some state (the caller falls back to one evaluation at a time, which sorts out which tables to drop).
// States per tile of the batched <H> and its workgroup size: two states with 512 threads leave ONE workgroup per CU (8 waves)
// where the single-state kernel keeps two or three; measured at 24 qubits, B = 64 (ms per evaluation): see DESIGN.md §4
constexpr int SEC_BATCH_NB = 2;   // (sector_batch_ready sizes LDS for it)
constexpr int SEC_BATCH_H_THREADS = 1024;
// the batch's circuit sweeps: 512-thread workgroups that read their scatter indices when the tile is written (44 instead of 64 KB
// per workgroup at 24 qubits: three workgroups per CU; B = 64: 0.82 -> 0.70 ms per evaluation)
constexpr int SEC_BATCH_SWEEP_THREADS = 512;
int run_sector_energy_batch(ovqe_handle h, int64_t B, const double *theta, bool theta_on_device, double *energies, bool *ok) {
    constexpr int NT = SEC_BATCH_H_THREADS, NB = SEC_BATCH_NB;
    SectorEngine &E = h->sec;
    *ok = false;
    if (!sector_sweeps2_fits(E, SEC_BATCH_SWEEP_THREADS, false))
        return OVQE_OK;   // a tile the batched sweeps cannot hold: one evaluation at a time still works
    const size_t S = h->srots.size();
    const size_t stride = std::max<size_t>(E.K, E.pad_elems);
    // states per pass: the two state buffers stay below ~4 GB (and the launch grid inside its limits)
    int64_t chunk = std::max<int64_t>(NB, std::min<int64_t>(256, (int64_t)(((size_t)2 << 30) / (stride * sizeof(double)))));
    chunk -= chunk % NB;
    chunk = std::min<int64_t>(chunk, (B + NB - 1) / NB * NB);
    int rc = ensure(h, E.d_bbuf[0], (size_t)chunk * stride * sizeof(double));
    if (!rc) rc = ensure(h, E.d_bbuf[1], (size_t)chunk * stride * sizeof(double));
    if (!rc) rc = ensure(h, E.d_brp, (size_t)chunk * std::max<size_t>(S, 1) * sizeof(RotParam));
    if (!rc) rc = ensure(h, E.d_benergies, (size_t)chunk * sizeof(double));
    if (!rc && !theta_on_device) rc = ensure(h, h->d_theta, (size_t)chunk * std::max(1, h->K) * sizeof(double));
    const uint32_t ng = sector_h_groups(E);
    const size_t nparts = (size_t)ng * E.hs.size();
    if (!rc) rc = ensure(h, h->d_partials, (size_t)(chunk / NB) * nparts * NB * sizeof(double));
    if (!rc) rc = lds_opt_in<&k_sector_expect_batch<NT, NB>>(h, SEC_LDS_MAX);
    if (rc == OVQE_ERR_ALLOC) {   // no room for the state slices of a batch next to the tables: the serial path needs none of them
        for (DevBuf *b : {&E.d_bbuf[0], &E.d_bbuf[1], &E.d_brp, &E.d_benergies}) free_buf(*b);
        (void)hipGetLastError();
        return OVQE_OK;
    }
    if (rc) return rc;
    for (int64_t b0 = 0; b0 < B; b0 += chunk) {
        const int64_t nb = std::min<int64_t>(chunk, B - b0);
        const int64_t nbp = (nb + NB - 1) / NB * NB;   // a ragged tail evaluates its last state again
        const double *d_theta = theta + b0 * h->K;
        if (!theta_on_device) {
            HIPC(h, hipMemcpyAsync(h->d_theta.p, theta + b0 * h->K, (size_t)nb * h->K * sizeof(double), hipMemcpyHostToDevice, h->stream));
            d_theta = (const double *)h->d_theta.p;
        }
        if (S) {
            hipLaunchKernelGGL(k_resolve_rots_batch, dim3((unsigned)((S + 255) / 256), (unsigned)nb), dim3(256), 0, h->stream,
                               (const RotSpec *)h->d_rots.p, (int)S, d_theta, h->K, (RotParam *)E.d_brp.p);
            for (int64_t q = nb; q < nbp; ++q)   // the tail of a pass is filled with copies of its last state
                HIPC(h, hipMemcpyAsync((RotParam *)E.d_brp.p + (size_t)q * S, (const RotParam *)E.d_brp.p + (size_t)(nb - 1) * S,
                                       S * sizeof(RotParam), hipMemcpyDeviceToDevice, h->stream));
        }
        int last = 0;
        rc = sector_sweeps2(h, E, SEC_BATCH_SWEEP_THREADS, (double *)E.d_bbuf[0].p, (double *)E.d_bbuf[1].p, stride, (const RotParam *)E.d_brp.p, S,
                            (int)nbp, &last, false);
        if (rc) return rc;
        // state group = fastest grid index (the groups share a tile's elements through the caches)
        const bool zfast = nbp / NB <= 65535 && E.hs.size() <= 65535;
        hipLaunchKernelGGL((k_sector_expect_batch<NT, NB>),
                           zfast ? dim3((unsigned)(nbp / NB), ng, (unsigned)E.hs.size()) : dim3(ng, (unsigned)E.hs.size(), (unsigned)(nbp / NB)),
                           dim3(NT), sec_h_lds_bytes(std::max(E.h_max_tile, 1u), NB, (uint32_t)E.h_max_dict), h->stream, (const double *)E.d_bbuf[last].p, stride,
                           (const SecHSweep *)E.d_hdesc.p, (double *)h->d_partials.p, std::max(E.h_max_tile, 1u), zfast ? 1 : 0);
        double *d_out = theta_on_device ? energies + b0 : (double *)E.d_benergies.p;
        if (theta_on_device && nbp > nb) d_out = (double *)E.d_benergies.p;   // (room for the duplicated state)
        hipLaunchKernelGGL(k_sec_reduce_batch, dim3((unsigned)nbp), dim3(256), 0, h->stream, (const double *)h->d_partials.p, (int)nparts,
                           NB, h->ham.constant, d_out);
        HIPC(h, hipGetLastError());
        if (!theta_on_device)
            HIPC(h, hipMemcpyAsync(energies + b0, d_out, (size_t)nb * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        else if (d_out != energies + b0)
            HIPC(h, hipMemcpyAsync(energies + b0, d_out, (size_t)nb * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
        HIPC(h, hipMemcpyAsync(h->h_result + 1, E.d_flag.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIPC(h, hipStreamSynchronize(h->stream));
        int flag = 0;
        std::memcpy(&flag, h->h_result + 1, sizeof(int));
        if (flag) {
            HIPC(h, hipMemsetAsync(E.d_flag.p, 0, sizeof(int), h->stream));   // the serial path re-raises it on its own evaluation
            return OVQE_OK;
        }
    }
    *ok = true;
    return OVQE_OK;
}

// dE/dtheta for all parameters on the sector tables (adjoint method): forward circuit, lambda = H psi on the support, one
// backward pass.  *ok as run_sector_energy.
template <int NT>
int launch_sector_adjoint(ovqe_handle h, SectorEngine &E, int last) {
    if (int rc = lds_opt_in<&k_sector_adjoint<NT>>(h, LDS_WG_MAX)) return rc;
    int cur = last, lcur = 0;   // psi in d_buf[cur], lambda in d_lam[lcur]
    for (int s = (int)E.segs.size() - 1; s >= 0; --s) {
        const SectorSeg &sg = E.segs[s];
        const uint32_t cap = std::max(sg.L.max_tile, 1u);
        const size_t smem = sec_adjoint_lds(cap, sg.nrot, sg.nops, NT / 64).bytes;
        if (smem > LDS_WG_MAX) return fail(h, OVQE_ERR_INVALID, "internal: sector adjoint tile exceeds LDS");
        h->forms_used |= 16u | secf_wg(SECF_WG_ADJOINT, NT);
        hipLaunchKernelGGL((k_sector_adjoint<NT>), dim3(sg.L.ntiles), dim3(NT), smem, h->stream, (const double *)E.d_buf[cur].p,
                           (const double *)E.d_lam[lcur].p, (double *)E.d_buf[cur ^ 1].p, (double *)E.d_lam[lcur ^ 1].p,
                           s ? (const uint32_t *)sg.L.d_src.p : (const uint32_t *)nullptr, (const uint32_t *)sg.L.d_off.p,
                           (const int32_t *)sg.d_tab0.p, sg.nops, (const uint32_t *)sg.d_poff.p, (const uint32_t *)sg.d_pairs.p,
                           (const RotParam *)h->d_rp.p, sg.rot0, sg.nrot, cap, (double *)E.d_wpart.p, (int)h->srots.size(), E.sb);
        cur ^= 1;
        lcur ^= 1;
    }
    const int S = (int)h->srots.size();
    hipLaunchKernelGGL(k_sec_reduce_w, dim3((unsigned)((S + 63) / 64)), dim3(256), 0, h->stream, (const double *)E.d_wpart.p,
                       E.segs[0].L.ntiles, S, (double *)E.d_w.p);
    HIPC(h, hipGetLastError());
    return OVQE_OK;
}

// second form (k_sector_adjoint2, 1024 threads) and third (k_sector_adjoint3, on the per-wave streams)
bool sector_adjoint2_fits(ovqe_handle h, const SectorEngine &E) {
    if (h->opt_sector_adjoint < 2 || h->opt_sector_sweep < 2 || !E.pad_elems || E.segs.empty()) return false;
    for (size_t s = 0; s < E.segs.size(); ++s) {
        const SectorSeg &sg = E.segs[s];
        if (!sg.d_wide.p || (s && !sg.d_bdst.p) || sg.maxchunks > 1024u ||
            sec_adjoint2_lds(std::max(sg.L.max_tile, 1u), sg.nrot, 1024 / 64, sg.maxchunks).bytes > LDS_WG_MAX)
            return false;
    }
    return true;
}
int launch_sector_adjoint2(ovqe_handle h, SectorEngine &E, int last) {
    constexpr int NT = 1024, WPT = 2;
    if (int rc = lds_opt_in<&k_sector_adjoint2<NT, WPT>>(h, LDS_WG_MAX)) return rc;
    int cur = last, lcur = 0;   // psi in d_buf[cur], lambda in d_lam[lcur]
    for (int s = (int)E.segs.size() - 1; s >= 0; --s) {
        const SectorSeg &sg = E.segs[s];
        const uint32_t cap = std::max(sg.L.max_tile, 1u);
        // third form: one row of partial sums per wave that shares the rows, no round counts
        const size_t smem3 = sec_adjoint2_lds(cap, sg.nrot, std::max(sg.stream_waves, 1), 0).bytes;
        if (sg.nruns > 0 && h->opt_sector_sweep >= 3 && h->opt_sector_adjoint >= 3 && smem3 <= LDS_WG_MAX) {   // on the per-wave streams
            if (int rc = lds_opt_in<&k_sector_adjoint3<NT>>(h, LDS_WG_MAX)) return rc;
            h->forms_used |= 64u | secf_wg(SECF_WG_ADJOINT, NT);
            hipLaunchKernelGGL((k_sector_adjoint3<NT>), dim3(sg.L.ntiles), dim3(NT), smem3, h->stream,
                               (const double *)E.d_buf[cur].p, (const double *)E.d_lam[lcur].p, (double *)E.d_buf[cur ^ 1].p,
                               (double *)E.d_lam[lcur ^ 1].p, s + 1 == (int)E.segs.size() ? 1 : 0,
                               s ? (const uint32_t *)sg.d_bdst.p : (const uint32_t *)nullptr, (const uint32_t *)sg.L.d_off.p,
                               (const uint32_t *)sg.d_rowinfo.p, sg.nruns, sg.stream_waves, (const uint32_t *)sg.d_stream.p,
                               (const uint16_t *)sg.d_rowhdr.p, (const RotParam *)h->d_rp.p, sg.rot0, sg.nrot, cap,
                               (double *)E.d_wpart.p, (int)h->srots.size(), E.sb);
            cur ^= 1;
            lcur ^= 1;
            continue;
        }
        h->forms_used |= 32u | secf_wg(SECF_WG_ADJOINT, NT);
        hipLaunchKernelGGL((k_sector_adjoint2<NT, WPT>), dim3(sg.L.ntiles), dim3(NT),
                           sec_adjoint2_lds(cap, sg.nrot, NT / 64, sg.maxchunks).bytes, h->stream,
                           (const double *)E.d_buf[cur].p, (const double *)E.d_lam[lcur].p, (double *)E.d_buf[cur ^ 1].p,
                           (double *)E.d_lam[lcur ^ 1].p, s + 1 == (int)E.segs.size() ? 1 : 0,
                           s ? (const uint32_t *)sg.d_bdst.p : (const uint32_t *)nullptr, (const uint32_t *)sg.L.d_off.p,
                           (const uint32_t *)sg.d_poff.p, sg.nops, (const uint64_t *)sg.d_wide.p, (const uint16_t *)sg.d_rounds.p,
                           sg.maxchunks, (const RotParam *)h->d_rp.p, sg.rot0, sg.nrot, cap,
                           (double *)E.d_wpart.p, (int)h->srots.size());
        cur ^= 1;
        lcur ^= 1;
    }
    const int S = (int)h->srots.size();
    hipLaunchKernelGGL(k_sec_reduce_w, dim3((unsigned)((S + 63) / 64)), dim3(256), 0, h->stream, (const double *)E.d_wpart.p,
                       E.segs[0].L.ntiles, S, (double *)E.d_w.p);
    HIPC(h, hipGetLastError());
    return OVQE_OK;
}

// the backward sweeps hold psi and lambda of a tile in LDS, plus one partial sum per wave and table entry: the largest
// workgroup size (<= want) whose sweeps all fit, 0 if none does
int sector_adjoint_threads(ovqe_handle h, int want) {
    const SectorEngine &E = h->sec;
    for (int nt : {1024, 512, 256}) {
        if (nt > want) continue;
        bool fits = true;
        for (const SectorSeg &sg : E.segs) fits = fits && sec_adjoint_lds(std::max(sg.L.max_tile, 1u), sg.nrot, sg.nops, nt / 64).bytes <= LDS_WG_MAX;
        if (fits) return nt;
    }
    return 0;
}
// backward sweeps of a regular support (k_sector_adjoint_reg; LDS: sec_reg_lds with psi's and lambda's tile).
// units of a run whose rows wait in LDS: as many as keep two workgroups on a CU (80 KB each), 1..16
int sector_adjoint_reg_runcap(const SectorEngine &E, const SectorSeg &sg, int nt) {
    const size_t base = sec_reg_lds(E.reg_m, 2, sg.nops, nt / 64, 0).bytes, per = sec_reg_lds(E.reg_m, 2, sg.nops, nt / 64, 1).bytes - base;
    const size_t room = base < LDS_TWO_PER_CU ? LDS_TWO_PER_CU - base : 0;
    return (int)std::max<size_t>(1, std::min<size_t>(16, room / per));
}
bool sector_adjoint_reg_fits(ovqe_handle h, const SectorEngine &E) {
    if (!h->opt_sector_regular || !sector_reg_fits(E)) return false;
    for (const SectorSeg &sg : E.segs)
        if (sec_reg_lds(E.reg_m, 2, sg.nops, 256 / 64, 1).bytes > LDS_WG_MAX) return false;
    return true;
}
int launch_sector_adjoint_reg(ovqe_handle h, SectorEngine &E, int last) {
    constexpr int NT = 256;
    size_t wmax = 1;
    for (const SectorSeg &sg : E.segs) wmax = std::max(wmax, (size_t)sg.L.ntiles * sg.nops * 8);
    int rc = lds_opt_in<&k_sector_adjoint_reg<NT>>(h, LDS_WG_MAX);
    if (!rc) rc = ensure(h, E.d_wpart, wmax * sizeof(double));
    if (rc) return rc;
    HIPC(h, hipMemsetAsync(E.d_w.p, 0, std::max<size_t>(h->srots.size(), 1) * sizeof(double), h->stream));
    int cur = last, lcur = 0;   // psi in E.d_buf[cur], lambda in E.d_lam[lcur], both in the last sweep's (canonical) order
    for (size_t si = E.segs.size(); si-- > 0;) {
        const SectorSeg &sg = E.segs[si];
        const int runcap = (E.reg_plan_threads == NT && h->opt_sector_reg_runs) ? sector_adjoint_reg_runcap(E, sg, NT) : 1;
        h->forms_used |= 128u | secf_wg(SECF_WG_REGULAR, NT);
        hipLaunchKernelGGL((k_sector_adjoint_reg<NT>), dim3(sg.L.ntiles), dim3(NT), sec_reg_lds(E.reg_m, 2, sg.nops, NT / 64, runcap).bytes, h->stream,
                           (const double *)E.d_buf[cur].p, (const double *)E.d_lam[lcur].p, (double *)E.d_buf[cur ^ 1].p,
                           (double *)E.d_lam[lcur ^ 1].p,
                           si ? (const uint32_t *)(sg.d_regsrc.p ? sg.d_regsrc.p : sg.d_srcpad.p) : (const uint32_t *)nullptr,
                           (const uint16_t *)sg.d_reggslot.p, (const uint16_t *)sg.d_regoslot.p, (const SecRegOp *)sg.d_regops.p, sg.nops,
                           (const uint32_t *)sg.d_reggw.p, (const double2 *)E.d_regtab.p + sg.regtab0, E.reg_m, (double *)E.d_wpart.p, runcap);
        hipLaunchKernelGGL(k_sec_reg_wreduce, dim3((unsigned)sg.nops * 8u), dim3(256), 0, h->stream, (const double *)E.d_wpart.p, sg.L.ntiles,
                           (uint32_t)sg.nops * 8u, (const uint32_t *)E.d_regmap.p + sg.regtab0, (double *)E.d_w.p);
        cur ^= 1;
        lcur ^= 1;
    }
    HIPC(h, hipGetLastError());
    return OVQE_OK;
}
bool sector_gradient_fits(ovqe_handle h) {
    return sector_adjoint_reg_fits(h, h->sec) || sector_adjoint2_fits(h, h->sec) || sector_adjoint_threads(h, 1024) != 0;
}

int run_sector_gradient(ovqe_handle h, const double *theta, double *energy, double *grad, bool *ok) {
    SectorEngine &E = h->sec;
    *ok = false;
    const size_t S = h->srots.size();
    const bool regular = sector_adjoint_reg_fits(h, E) && h->opt_sector_reg_adjoint;
    const bool second = !regular && sector_adjoint2_fits(h, E);
    const size_t lam_elems = second ? std::max<size_t>(E.K, E.pad_elems) : (size_t)E.K;
    int rc = ensure(h, E.d_lam[0], lam_elems * sizeof(double));
    if (!rc) rc = ensure(h, E.d_lam[1], lam_elems * sizeof(double));
    if (!rc) rc = ensure(h, E.d_w, std::max<size_t>(S, 1) * sizeof(double));
    const size_t wpart_bytes = regular ? 256 : (size_t)E.segs[0].L.ntiles * std::max<size_t>(S, 1) * sizeof(double);   // (regular: sized per sweep by its launcher)
    if (!rc) rc = ensure(h, E.d_wpart, wpart_bytes);
    const int nbd = (int)std::min<uint32_t>(1024u, (E.K + 255u) / 256u);
    if (!rc) rc = ensure(h, h->d_partials, (size_t)nbd * sizeof(double2));
    if (!rc) rc = ensure(h, h->d_result, 64 * sizeof(double2));
    if (rc) return rc;
    int last = 0;
    rc = run_sector_circuit(h, theta, &last);
    if (rc) return rc;
    HIPC(h, hipMemsetAsync(E.d_wpart.p, 0, wpart_bytes, h->stream));
    rc = sector_matvec(h, E, (const double *)E.d_buf[last].p, (double *)E.d_lam[0].p);
    if (rc) return rc;
    hipLaunchKernelGGL(k_sec_dot, dim3(nbd), dim3(256), 0, h->stream, (const double *)E.d_buf[last].p, (const double *)E.d_lam[0].p,
                       E.K, (double2 *)h->d_partials.p);
    if ((rc = enqueue_reduce(h, h->d_partials.p, nbd))) return rc;
    if (regular) {
        rc = launch_sector_adjoint_reg(h, E, last);
    } else if (second) {
        rc = launch_sector_adjoint2(h, E, last);
    } else {
        int nthr = h->opt_sector_threads;
        if (nthr == 0) {
            const double avg = (double)E.K / (double)std::max<uint64_t>(1, h->namps >> E.M);
            nthr = avg >= 1500.0 ? 1024 : (avg >= 600.0 ? 512 : 256);
        }
        nthr = sector_adjoint_threads(h, std::max(nthr, 256));
        switch (nthr) {
        case 512: rc = launch_sector_adjoint<512>(h, E, last); break;
        case 1024: rc = launch_sector_adjoint<1024>(h, E, last); break;
        default: rc = launch_sector_adjoint<256>(h, E, last); break;
        }
    }
    if (rc) return rc;
    std::vector<double> w(S, 0.0);
    HIPC(h, hipMemcpyAsync(h->h_result, h->d_result.p, sizeof(double2), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipMemcpyAsync(h->h_result + 1, E.d_flag.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (S) HIPC(h, hipMemcpyAsync(w.data(), E.d_w.p, S * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    int flag = 0;
    std::memcpy(&flag, h->h_result + 1, sizeof(int));
    if (flag) return OVQE_OK;
    for (int32_t p = 0; p < h->K; ++p) grad[p] = 0.0;
    for (size_t r = 0; r < S; ++r) {
        const SmallRot &sr = h->srots[r];
        if (sr.pidx >= 0) grad[sr.pidx] += 2.0 * sr.coeff * ((sr.ny & 2) ? -w[r] : w[r]);
    }
    *energy = h->h_result[0].x + h->ham.constant;
    *ok = true;
    return OVQE_OK;
}

// Lowest eigenpair of the Hamiltonian RESTRICTED TO THE SUPPORT of the stored program's states (for a number- and
// spin-conserving ansatz on a Hartree-Fock determinant: the FCI energy of that symmetry sector), by two-pass Lanczos on
// the sector tables: the matrix-vector product is lambda = H v of the gradient path.
int sector_matvec(ovqe_handle h, SectorEngine &E, const double *in, double *out) {
    // lambda needs a second tile in LDS: where that leaves one 512-thread workgroup per CU (expect: two or three), 1024 threads
    // keep 16 waves on the CU (24 qubits: 1.33 -> 1.19 ms per pass).  Round 5: with two loads in flight per lane instead of four the
    // kernel needs 109 registers (161 before: the 1024-thread form spilled 24 of them) and 1024 threads also win where two 512-thread
    // workgroups would fit (N2 QUCCSD tables, tiles of 4096: gradient 14.2 -> 13.8 ms; UCCSD 2.91 -> 2.83 ms)
    const size_t smem = sec_h_lds_bytes(std::max(E.h_max_tile, 1u), 2, (uint32_t)E.h_max_dict);
    const int nt = smem > 48 * 1024 ? 1024 : 512;
    // one launch per sweep, in sequence: no global atomics (k_sector_apply, modes 1 / 2), the first sweep stores; every support
    // entry sits in exactly one tile of every sweep, so sweep 0's stores cover the whole vector (no memset)
    const unsigned nsw = (unsigned)E.hs.size();
    // (only where ONE sweep fills the chip: the N2 UCCSD tables have 83 tiles per sweep — seven sweeps side by side 3.3 ms per gradient,
    // in sequence 4.1; the QUCCSD tables 1024 per sweep: 14.9 -> 14.2 ms)
    const bool seq = nsw >= 1 && (uint64_t)E.K >= 512ull * std::max(E.h_max_tile, 1u);
    if (!seq) HIPC(h, hipMemsetAsync(out, 0, (size_t)E.K * sizeof(double), h->stream));
    const dim3 grid(sector_h_groups(E), seq ? 1u : nsw);
    for (unsigned s0 = 0; s0 < (seq ? nsw : 1u); ++s0) {
        const int mode = seq ? (s0 == 0 ? 2 : 1) : 0;
        h->forms_used |= (seq ? SECF_APPLY_SEQ : SECF_APPLY_ATOMIC) | (nt == 1024 ? SECF_APPLY_1024 : SECF_APPLY_512);
        if (nt == 1024) {
            if (int rc = lds_opt_in<&k_sector_apply<1024>>(h, SEC_LDS_MAX)) return rc;
            hipLaunchKernelGGL((k_sector_apply<1024>), grid, dim3(1024), smem, h->stream, in, (const SecHSweep *)E.d_hdesc.p, out,
                               std::max(E.h_max_tile, 1u), (int)s0, mode);
        } else {
            if (int rc = lds_opt_in<&k_sector_apply<SEC_H_THREADS>>(h, SEC_LDS_MAX)) return rc;
            hipLaunchKernelGGL((k_sector_apply<SEC_H_THREADS>), grid, dim3(SEC_H_THREADS), smem, h->stream, in, (const SecHSweep *)E.d_hdesc.p,
                               out, std::max(E.h_max_tile, 1u), (int)s0, mode);
        }
    }
    HIPC(h, hipGetLastError());
    return OVQE_OK;
}

// The compact support as a Lanczos space (sv_lanczos_host.hpp): vectors are K doubles, the operator is sector_matvec, and the start vector
// and every update are projected on `reach`, the 0/1 mask of the block of H connected to the reference determinant.  Two-pass only.
struct SectorSpace : LanczosTwoPass {
    typedef double *Vec;
    ovqe_handle h;
    SectorEngine &E;
    DevBuf *vec;   // v_{j-1}, v_j, w, Ritz vector, reach
    uint64_t seed;
    const uint32_t K = E.K;
    const int nb = (int)std::min<uint32_t>(1024u, (K + 255u) / 256u);
    const double *reach = (const double *)vec[4].p;
    SectorSpace(ovqe_handle h, SectorEngine &E, DevBuf *vec, uint64_t seed) : h(h), E(E), vec(vec), seed(seed) {}
    Vec work(int i) const { return (double *)vec[i].p; }
    Vec ritz() const { return (double *)vec[3].p; }
    int reduce(double *out) { return reduce_to_host(h, h->d_partials.p, nb, out); }
    int start(Vec v) {
        hipLaunchKernelGGL(k_sec_randomize, dim3(nb), dim3(256), 0, h->stream, v, reach, K, seed, (double2 *)h->d_partials.p);
        double n2 = 0.0;
        if (int rc = reduce(&n2)) return rc;
        return scale(v, 1.0 / std::sqrt(n2));
    }
    int apply(Vec out, Vec in) { return sector_matvec(h, E, in, out); }
    int dot(Vec a, Vec b, double *re) {
        hipLaunchKernelGGL(k_sec_dot, dim3(nb), dim3(256), 0, h->stream, (const double *)a, (const double *)b, K, (double2 *)h->d_partials.p);
        return reduce(re);
    }
    int update(Vec w, Vec v, Vec vprev, double alpha, double beta, double *norm2) {
        hipLaunchKernelGGL(k_sec_lanczos_update, dim3(nb), dim3(256), 0, h->stream, w, (const double *)v, (const double *)vprev, alpha, beta, K,
                           (double2 *)h->d_partials.p, reach);
        return reduce(norm2);
    }
    int scale(Vec v, double a) {
        hipLaunchKernelGGL(k_sec_scale, dim3(nb), dim3(256), 0, h->stream, v, K, a);
        return OVQE_OK;
    }
    int axpy(Vec y, Vec x, double a, bool first) {
        hipLaunchKernelGGL(k_sec_axpy, dim3(nb), dim3(256), 0, h->stream, y, (const double *)x, a, K, first ? 1 : 0);
        return OVQE_OK;
    }
};

int run_sector_ground_state(ovqe_handle h, SectorEngine &E, double tol, int max_iter, uint64_t seed, double *energy, double *residual,
                            int *iterations) {
    const uint32_t K = E.K;
    const int nb = (int)std::min<uint32_t>(1024u, (K + 255u) / 256u);
    int rc = ensure(h, h->d_partials, (size_t)nb * sizeof(double2));
    if (!rc) rc = ensure(h, h->d_result, 64 * sizeof(double2));
    DevBuf vec[5];   // v_{j-1}, v_j, w, Ritz vector, reachability from the reference determinant
    for (DevBuf &b : vec)
        if (!rc) rc = ensure(h, b, (size_t)K * sizeof(double));
    auto cleanup = [&](int code) {
        for (DevBuf &b : vec) free_buf(b);
        return code;
    };
    if (rc) return cleanup(rc);
    SectorSpace V(h, E, vec, seed);
    // The support may be a superset of the reference determinant's symmetry sector (tables from the one-angle-per-rotation
    // probe hold every determinant the program can touch): Lanczos runs inside the block of H connected to |hf>, found here
    double *reach = (double *)vec[4].p;
    uint32_t members = 0;
    {
        double hmax = 0.0;
        for (const HTerm &ht : h->ham.terms) hmax = std::max(hmax, std::max(std::fabs(ht.cr), std::fabs(ht.ci)));
        const double reach_thresh = 1e-11 * hmax;
        hipLaunchKernelGGL(k_sec_reach_init, dim3(nb), dim3(256), 0, h->stream, reach, K, E.hf_final);
        double cnt = 1.0, prev = 0.0;
        // rounds to saturation: a molecular two-body H connects its sector in a few, a short-range one (hopping chain)
        // needs as many as the diameter of its determinant graph — at most one new member per round in the worst case
        const int max_rounds = (int)std::min<uint32_t>(K, 1u << 16);
        int it = 0;
        for (; it <= max_rounds && cnt != prev; ++it) {
            prev = cnt;
            rc = sector_matvec(h, E, reach, (double *)vec[2].p);
            if (rc) return cleanup(rc);
            hipLaunchKernelGGL(k_sec_reach_step, dim3(nb), dim3(256), 0, h->stream, reach, (const double *)vec[2].p, K,
                               0x5ec70full + (uint64_t)it, reach_thresh, (double2 *)h->d_partials.p);
            rc = V.reduce(&cnt);
            if (rc) return cleanup(rc);
        }
        if (cnt != prev)   // never diagonalise a truncated block: the number would lie above the sector's minimum
            return cleanup(fail(h, OVQE_ERR_STATE, "sector_ground_state: the block of H connected to the reference determinant did not "
                                                   "saturate within " + std::to_string(max_rounds) + " rounds"));
        members = (uint32_t)cnt;
        E.last_fci_block = members;
        E.last_fci_rounds = it;
        h->last_fci_rounds = it;
    }
    max_iter = (int)std::min<uint64_t>((uint64_t)max_iter, std::max(members, 1u));
    LanczosResult res;
    rc = lanczos_lowest(V, tol, max_iter, res);
    const bool canonical = E.segs.empty();   // an engine without a circuit (build_screen_sector) keeps its vectors in ascending-index order
    if (!rc && h->state && (canonical || E.segs.back().L.d_cid.p)) {
        // the normalised eigenvector as the handle's state (zeros outside the support), like ovqe_ground_state leaves it
        if (hipMemsetAsync(h->state, 0, (size_t)h->namps * sizeof(amp_t), h->stream) != hipSuccess) rc = fail(h, OVQE_ERR_HIP, "sector_ground_state: memset");
        if (!rc)
            hipLaunchKernelGGL(k_sec_scatter_dense, dim3((K + 255u) / 256u), dim3(256), 0, h->stream, (const double *)V.ritz(),
                               canonical ? (const uint32_t *)nullptr : (const uint32_t *)E.segs.back().L.d_cid.p, (const uint32_t *)E.d_sup.p, K,
                               (double2 *)h->state);
        if (!rc && hipStreamSynchronize(h->stream) != hipSuccess) rc = fail(h, OVQE_ERR_HIP, "sector_ground_state: scatter");
    }
    if (!rc && hipGetLastError() != hipSuccess) rc = fail(h, OVQE_ERR_HIP, "sector_ground_state: launch failed");
    if (rc) return cleanup(rc);
    *energy = res.lam + h->ham.constant;
    if (residual) *residual = res.residual;
    if (iterations) *iterations = res.m;
    return cleanup(OVQE_OK);
}
