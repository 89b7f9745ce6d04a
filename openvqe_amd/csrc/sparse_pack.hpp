// sparse_pack.hpp — the restricted Hamiltonian as OWNER PIECES for k_sparse_vqe_rows_shared (sv_sparse.hpp).
//
// The entries (i, j, c) of the restricted Hamiltonian are a symmetric quadratic form: E = sum_i a_i (sum_{j in row i} c_ij a_j).
// Every off-diagonal entry may be owned by either endpoint, the diagonal entry of row i is owned by i (j = i, c = H_ii: the same
// c a_i a_i, no special case).  A PIECE is up to EPR entries of one owner; thread t holds RPT pieces.  Per piece and state the
// kernel reads a_owner once and one a_j per slot — EPR + 1 LDS reads and EPR + 1 fma instead of 2 EPR reads and 2 EPR operations.
//
// Pure host code on plain vectors (no HIP): tests/test_sparse_pack.py compiles it into a host program.  The order is a function
// of the entry list alone: energies stay reproducible.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "sparse_plan.hpp"

namespace ovqe {

struct OwnerPack {
    int nt = 0, rpt = 0, epr = 0;
    int pieces = 0;              // sum over the rows of ceil(load / EPR): the pieces that hold entries (<= nt * rpt)
    std::vector<uint16_t> oi;    // [rpt][nt]        byte offset of the piece's owner amplitude
    std::vector<uint16_t> oj;    // [rpt * epr][nt]  byte offset of the slot's other amplitude (padding: the owner's)
    std::vector<double> c;       // [rpt * epr][nt]  coefficient (padding and empty pieces: 0)
};

// One slot of a piece as instruction k of a group of 32 lanes reads it.
struct PackSlot {
    uint32_t o;   // the slot read
    double c;
    int real;     // 0: padding (c = 0; the owner's slot, or the one slot of an empty piece)
};

// The order of the slots inside the pieces of ONE group of 32 lanes.  in: tab[l] the entries of lane l's piece (at most epr; own[l]
// its owner, 0xffffffff: an empty piece).  out: tab[l] of exactly epr slots, own[l] a valid slot for every lane.
// Instruction k reads tab[.][k]: one LDS cycle when the slots differ mod 32 (equal slots are one word).  The lanes and the 32
// banks are the two sides of a bipartite multigraph with one edge per slot, an order of the slots is a colouring of its edges with
// epr colours, and an instruction without conflict is a colour that no bank sees twice.  When no bank carries more than epr edges
// such a colouring exists (Koenig) and alternating paths find it: first with the padding counted (a tail reads its owner's slot,
// an empty piece ONE slot on the least loaded bank), else for the entries alone with the padding in the colours they leave.  What
// conflicts remain goes to a local search on the model: two slots of one lane change places when that shortens the two instructions
// together.  A bank with more than epr edges need not cost anything — lanes that read the SAME slot in one instruction read one word,
// and a restricted Hamiltonian has slots that most pieces of a group read — but then a slot's instruction ties lanes together and
// the problem is no edge colouring any more: the start is greedy (the most shared slots first), the rest the same search.
inline void pack_group_slots(std::vector<PackSlot> (&tab)[32], uint32_t (&own)[32], int nslots, int epr) {
    int deg[32] = {}, deg_real[32] = {};
    for (int l = 0; l < 32; ++l) {
        if (own[l] == 0xffffffffu) continue;
        for (const PackSlot &s : tab[l]) {
            ++deg[s.o & 31u];
            ++deg_real[s.o & 31u];
        }
        deg[own[l] & 31u] += epr - (int)tab[l].size();
    }
    for (int l = 0; l < 32; ++l) {
        if (own[l] != 0xffffffffu) continue;
        uint32_t best = 0;
        for (uint32_t s = 1; s < (uint32_t)std::min(nslots, 32); ++s)
            if (deg[s & 31u] < deg[best & 31u]) best = s;
        own[l] = best;
        deg[best & 31u] += epr;
    }
    for (int l = 0; l < 32; ++l)
        while ((int)tab[l].size() < epr) tab[l].push_back({own[l], 0.0, 0});
    int worst = 0, worst_real = 0;
    for (int b = 0; b < 32; ++b) {
        worst = std::max(worst, deg[b]);
        worst_real = std::max(worst_real, deg_real[b]);
    }
    const bool all = worst <= epr, reals = !all && worst_real <= epr;
    if (all || reals) {
        // edge (l, q) = tab[l][q] as it stands; colour[l][q] = the instruction that reads it
        std::vector<int> colour((size_t)32 * epr, -1), at_lane((size_t)32 * epr, -1), at_bank((size_t)32 * epr, -1);   // [.][colour] -> edge l * epr + q
        auto bank_of = [&](int e) { return (int)(tab[e / epr][(size_t)(e % epr)].o & 31u); };
        auto put = [&](int e, int col) {
            colour[(size_t)e] = col;
            at_lane[(size_t)(e / epr) * epr + col] = e;
            at_bank[(size_t)bank_of(e) * epr + col] = e;
        };
        std::vector<int> path;
        for (int l = 0; l < 32; ++l)
            for (int q = 0; q < epr; ++q) {
                if (!all && !tab[l][(size_t)q].real) continue;
                const int e = l * epr + q, b = bank_of(e);
                int ca = 0, cb = 0;
                while (at_lane[(size_t)l * epr + ca] >= 0) ++ca;   // free at the lane (its degree is at most epr)
                while (at_bank[(size_t)b * epr + cb] >= 0) ++cb;   // free at the bank
                if (at_bank[(size_t)b * epr + ca] >= 0) {
                    // the path from the bank along colours ca, cb, ca, ...: it cannot reach lane l (every lane on it is entered on ca)
                    path.clear();
                    for (int bb = b;;) {
                        const int e1 = at_bank[(size_t)bb * epr + ca];
                        if (e1 < 0) break;
                        path.push_back(e1);
                        const int e2 = at_lane[(size_t)(e1 / epr) * epr + cb];
                        if (e2 < 0) break;
                        path.push_back(e2);
                        bb = bank_of(e2);
                    }
                    for (int f : path) {
                        at_lane[(size_t)(f / epr) * epr + colour[(size_t)f]] = -1;
                        at_bank[(size_t)bank_of(f) * epr + colour[(size_t)f]] = -1;
                    }
                    for (int f : path) put(f, colour[(size_t)f] == ca ? cb : ca);
                }
                put(e, ca);
            }
        for (int l = 0; l < 32; ++l) {
            std::vector<PackSlot> ordered((size_t)epr, PackSlot{own[l], 0.0, 0});
            std::vector<char> filled((size_t)epr, 0);
            for (int q = 0; q < epr; ++q)
                if (colour[(size_t)l * epr + q] >= 0) {
                    ordered[(size_t)colour[(size_t)l * epr + q]] = tab[l][(size_t)q];
                    filled[(size_t)colour[(size_t)l * epr + q]] = 1;
                }
            int k = 0;
            for (int q = 0; q < epr; ++q)
                if (colour[(size_t)l * epr + q] < 0) {   // padding into the colours left
                    while (filled[(size_t)k]) ++k;
                    ordered[(size_t)k] = tab[l][(size_t)q];
                    filled[(size_t)k] = 1;
                }
            tab[l].swap(ordered);
        }
        if (all) return;
    }
    if (!all && !reals) {
        // no exact colouring: the slots that most lanes share first, each into the instruction where its bank is free and most of its
        // lanes still are (they read ONE word there), what finds no such instruction into the colours left
        struct Want { uint32_t o; std::vector<int> lanes; };
        std::vector<Want> wants;
        {
            std::vector<std::pair<uint32_t, int>> sl;
            for (int l = 0; l < 32; ++l)
                for (const PackSlot &s : tab[l])
                    if (s.real) sl.push_back({s.o, l});
            std::sort(sl.begin(), sl.end());
            for (size_t k = 0; k < sl.size(); ++k) {
                if (!k || sl[k].first != sl[k - 1].first) wants.push_back({sl[k].first, {}});
                wants.back().lanes.push_back(sl[k].second);
            }
            std::stable_sort(wants.begin(), wants.end(), [](const Want &a, const Want &b) { return a.lanes.size() > b.lanes.size(); });
        }
        std::vector<int> lane_free((size_t)32 * epr, 1), bank_slot((size_t)epr * 32, -1);
        std::vector<PackSlot> placed[32];
        for (int l = 0; l < 32; ++l) placed[l].assign((size_t)epr, PackSlot{own[l], 0.0, -1});   // real = -1: colour not taken
        auto coeff = [&](int l, uint32_t o) {
            for (const PackSlot &s : tab[l])
                if (s.real && s.o == o) return s.c;
            return 0.0;
        };
        std::vector<std::pair<int, uint32_t>> rest;   // (lane, slot) without an instruction
        for (Want &w : wants) {
            std::vector<int> left = w.lanes;
            while (!left.empty()) {
                int best = -1, best_n = 0;
                for (int k = 0; k < epr; ++k) {
                    const int held = bank_slot[(size_t)k * 32 + (w.o & 31u)];
                    if (held >= 0 && (uint32_t)held != w.o) continue;
                    int n = 0;
                    for (int l : left) n += lane_free[(size_t)l * epr + k];
                    if (n > best_n) {
                        best_n = n;
                        best = k;
                    }
                }
                if (best < 0) break;
                bank_slot[(size_t)best * 32 + (w.o & 31u)] = (int)w.o;
                std::vector<int> still;
                for (int l : left)
                    if (lane_free[(size_t)l * epr + best]) {
                        lane_free[(size_t)l * epr + best] = 0;
                        placed[l][(size_t)best] = {w.o, coeff(l, w.o), 1};
                    } else {
                        still.push_back(l);
                    }
                left.swap(still);
            }
            for (int l : left) rest.push_back({l, w.o});
        }
        for (auto &lo : rest)
            for (int k = 0; k < epr; ++k)
                if (lane_free[(size_t)lo.first * epr + k]) {
                    lane_free[(size_t)lo.first * epr + k] = 0;
                    placed[lo.first][(size_t)k] = {lo.second, coeff(lo.first, lo.second), 1};
                    break;
                }
        for (int l = 0; l < 32; ++l) {
            for (PackSlot &s : placed[l])
                if (s.real < 0) s.real = 0;
            tab[l].swap(placed[l]);
        }
    }
    // local search.  First on the colliding pairs, sum over instructions and banks of d (d - 1) / 2 for d distinct slots — it
    // falls with every slot that leaves a crowded bank, where the cycle count (the largest d of an instruction) stays flat —
    // then on the model's cycles themselves, for what the first leaves on a plateau of the second.
    std::vector<uint32_t> ids;
    for (int l = 0; l < 32; ++l)
        for (const PackSlot &s : tab[l]) ids.push_back(s.o);
    std::sort(ids.begin(), ids.end());
    ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    const size_t nid = ids.size();
    std::vector<int> id((size_t)32 * epr), refs((size_t)epr * nid, 0), dist((size_t)epr * 32, 0);
    int64_t q = 0;
    auto add = [&](int k, int i) {
        if (refs[(size_t)k * nid + (size_t)i]++ == 0) q += dist[(size_t)k * 32 + (ids[(size_t)i] & 31u)]++;
    };
    auto drop = [&](int k, int i) {
        if (--refs[(size_t)k * nid + (size_t)i] == 0) q -= --dist[(size_t)k * 32 + (ids[(size_t)i] & 31u)];
    };
    for (int l = 0; l < 32; ++l)
        for (int k = 0; k < epr; ++k) {
            id[(size_t)l * epr + k] = (int)(std::lower_bound(ids.begin(), ids.end(), tab[l][(size_t)k].o) - ids.begin());
            add(k, id[(size_t)l * epr + k]);
        }
    auto exchange = [&](int l, int k1, int k2) {
        int &a = id[(size_t)l * epr + k1], &b = id[(size_t)l * epr + k2];
        drop(k1, a);
        drop(k2, b);
        add(k1, b);
        add(k2, a);
        std::swap(a, b);
        std::swap(tab[l][(size_t)k1], tab[l][(size_t)k2]);
    };
    for (int sweep = 0; sweep < 64 && q > 0; ++sweep) {
        bool any = false;
        for (int l = 0; l < 32; ++l)
            for (int k1 = 0; k1 < epr; ++k1)
                for (int k2 = k1 + 1; k2 < epr; ++k2) {
                    if (id[(size_t)l * epr + k1] == id[(size_t)l * epr + k2]) continue;
                    const int64_t before = q;
                    exchange(l, k1, k2);
                    if (q < before)
                        any = true;
                    else
                        exchange(l, k1, k2);
                }
        if (!any) break;
    }
    auto cycles = [&](int k) {
        int worst = 0;
        for (int b = 0; b < 32; ++b) worst = std::max(worst, dist[(size_t)k * 32 + b]);
        return worst;
    };
    for (int sweep = 0; sweep < 8; ++sweep) {
        bool any = false;
        for (int k1 = 0; k1 < epr; ++k1)
            for (int l = 0; l < 32; ++l) {
                const int c1 = cycles(k1);
                if (c1 <= 1) break;
                if (dist[(size_t)k1 * 32 + (tab[l][(size_t)k1].o & 31u)] < c1) continue;   // (not on a bank that sets the cycles)
                for (int k2 = 0; k2 < epr; ++k2) {
                    if (k2 == k1 || id[(size_t)l * epr + k1] == id[(size_t)l * epr + k2]) continue;
                    const int c2 = cycles(k2);
                    const int64_t before = q;
                    exchange(l, k1, k2);
                    const int d = cycles(k1) + cycles(k2) - c1 - c2;
                    if (d < 0 || (d == 0 && q < before)) {
                        any = true;
                        break;
                    }
                    exchange(l, k1, k2);
                }
            }
        if (!any) break;
    }
}

// si, sj: slots (amplitude index in the LDS state, < nslots <= 8192), c: coefficient of c a_i a_j, every unordered pair at most
// once.  -> false when sum_i ceil(load_i / epr) > nt * rpt for the owners found (nothing usable in *out).
inline bool pack_owner_pieces(const std::vector<uint32_t> &si, const std::vector<uint32_t> &sj, const std::vector<double> &c, int nslots,
                              int nt, int rpt, int epr, OwnerPack *out) {
    const size_t n = si.size();
    out->nt = nt;
    out->rpt = rpt;
    out->epr = epr;
    out->pieces = 0;
    if (nslots < 1 || nslots > 8192 || nt < 32 || nt % 32 || rpt < 1 || epr < 1 || sj.size() != n || c.size() != n) return false;
    for (size_t e = 0; e < n; ++e)
        if (si[e] >= (uint32_t)nslots || sj[e] >= (uint32_t)nslots) return false;
    const int64_t capacity = (int64_t)nt * rpt;
    // ---- owners: balanced first (the endpoint with the smaller load), then whole pieces saved where a row's remainder fits into
    // the free slots of its neighbours' last pieces
    std::vector<int> load((size_t)nslots, 0);
    std::vector<uint32_t> owner(n);
    for (size_t e = 0; e < n; ++e)
        if (si[e] == sj[e]) {
            owner[e] = si[e];
            ++load[si[e]];
        }
    for (size_t e = 0; e < n; ++e)
        if (si[e] != sj[e]) {
            owner[e] = load[sj[e]] < load[si[e]] ? sj[e] : si[e];
            ++load[owner[e]];
        }
    auto pieces_of = [&](int l) { return (l + epr - 1) / epr; };
    int64_t pieces = 0;
    for (int i = 0; i < nslots; ++i) pieces += pieces_of(load[i]);
    if (pieces > capacity && epr > 1) {
        std::vector<std::vector<uint32_t>> owned((size_t)nslots);   // off-diagonal entries by owner
        for (size_t e = 0; e < n; ++e)
            if (si[e] != sj[e]) owned[owner[e]].push_back((uint32_t)e);
        auto slack = [&](int i) { return load[i] % epr ? epr - load[i] % epr : 0; };
        std::vector<int> order((size_t)nslots);
        std::vector<uint32_t> moved;
        for (int pass = 0; pass < 64 && pieces > capacity; ++pass) {
            const int64_t before = pieces;
            for (int i = 0; i < nslots; ++i) order[i] = i;
            std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return load[a] % epr < load[b] % epr; });   // small remainders first
            for (int i : order) {
                const int rem = load[i] % epr;
                if (!rem || pieces <= capacity) continue;
                // rem entries of row i to neighbours with a free slot in their last piece: one piece less, none more
                moved.clear();
                std::vector<uint32_t> &lst = owned[i];
                for (size_t k = 0; k < lst.size() && (int)moved.size() < rem; ++k) {
                    const uint32_t e = lst[k], o = si[e] == (uint32_t)i ? sj[e] : si[e];
                    int taken = 0;
                    for (uint32_t m : moved) taken += (si[m] == (uint32_t)i ? sj[m] : si[m]) == o;
                    if (slack((int)o) > taken) moved.push_back(e);
                }
                if ((int)moved.size() < rem) continue;
                for (uint32_t e : moved) {
                    const uint32_t o = si[e] == (uint32_t)i ? sj[e] : si[e];
                    lst.erase(std::find(lst.begin(), lst.end(), e));
                    owned[o].push_back(e);
                    owner[e] = o;
                    ++load[o];
                    --load[i];
                }
                --pieces;
            }
            if (pieces == before) break;
        }
    }
    if (pieces > capacity) return false;
    out->pieces = (int)pieces;
    // ---- pieces: the entries of a row in input order, EPR at a time
    struct Piece { uint32_t owner; std::vector<uint32_t> ent; };
    std::vector<Piece> pcs;
    {
        std::vector<std::vector<uint32_t>> by_owner((size_t)nslots);
        for (size_t e = 0; e < n; ++e) by_owner[owner[e]].push_back((uint32_t)e);
        for (int i = 0; i < nslots; ++i)
            for (size_t k0 = 0; k0 < by_owner[i].size(); k0 += (size_t)epr) {
                Piece p;
                p.owner = (uint32_t)i;
                p.ent.assign(by_owner[i].begin() + (long)k0, by_owner[i].begin() + (long)std::min(by_owner[i].size(), k0 + (size_t)epr));
                pcs.push_back(std::move(p));
            }
    }
    // ---- threads: an LDS read is served in aligned groups of 32 lanes, bank = slot mod 32.  Groups (piece r, 32 lanes) are filled one
    // after the other with pieces whose owners differ mod 32 where the set allows (fullest bank first), the rest with what is left
    out->oi.assign((size_t)rpt * nt, 0);
    out->oj.assign((size_t)rpt * epr * nt, 0);
    out->c.assign((size_t)rpt * epr * nt, 0.0);
    std::vector<std::vector<uint32_t>> by_bank(32);
    for (size_t p = pcs.size(); p-- > 0;) by_bank[pcs[p].owner & 31u].push_back((uint32_t)p);   // (taken from the back: input order)
    size_t left = pcs.size();
    std::vector<int> bank_order(32);
    for (int r = 0; r < rpt; ++r)
        for (int t0 = 0; t0 < nt; t0 += 32) {
            int32_t lane_piece[32];
            int taken = 0;
            for (int b = 0; b < 32; ++b) bank_order[b] = b;
            std::stable_sort(bank_order.begin(), bank_order.end(), [&](int a, int b) { return by_bank[a].size() > by_bank[b].size(); });
            for (int b : bank_order)
                if (!by_bank[b].empty()) {
                    lane_piece[taken++] = (int32_t)by_bank[b].back();
                    by_bank[b].pop_back();
                    --left;
                }
            // pieces that no later group has room for with a bank of their own
            const size_t room_behind = (size_t)(rpt - 1 - r) * nt + (size_t)(nt - 32 - t0);
            for (int b : bank_order)
                while (taken < 32 && left > room_behind && !by_bank[b].empty()) {
                    lane_piece[taken++] = (int32_t)by_bank[b].back();
                    by_bank[b].pop_back();
                    --left;
                }
            for (int l = taken; l < 32; ++l) lane_piece[l] = -1;
            // slots: which of a lane's entries instruction k reads (pack_group_slots above)
            std::vector<PackSlot> tab[32];
            uint32_t own[32];
            for (int l = 0; l < 32; ++l) {
                own[l] = 0xffffffffu;
                if (lane_piece[l] < 0) continue;
                const Piece &p = pcs[(size_t)lane_piece[l]];
                own[l] = p.owner;
                for (uint32_t e : p.ent) tab[l].push_back({si[e] == p.owner ? sj[e] : si[e], c[e], 1});
            }
            pack_group_slots(tab, own, nslots, epr);
            for (int l = 0; l < 32; ++l) {
                const size_t t = (size_t)t0 + l;
                out->oi[(size_t)r * nt + t] = (uint16_t)(own[l] * 8u);
                for (int k = 0; k < epr; ++k) {
                    const size_t at = ((size_t)r * epr + k) * nt + t;
                    out->oj[at] = (uint16_t)(tab[l][(size_t)k].o * 8u);
                    out->c[at] = tab[l][(size_t)k].c;
                }
            }
        }
    return left == 0;
}

// Modelled LDS array cycles of the contraction per state (sparse_plan.hpp: lds_access_cycles): every aligned group of 32 threads
// reads rpt * epr slots and rpt owners.
struct PackCycles { int64_t slot_reads = 0, owner_reads = 0; };
inline PackCycles pack_cycles(const OwnerPack &P) {
    PackCycles c;
    uint32_t s[32];
    for (int t0 = 0; t0 + 32 <= P.nt; t0 += 32) {
        for (int k = 0; k < P.rpt * P.epr; ++k) {
            for (int l = 0; l < 32; ++l) s[l] = P.oj[(size_t)k * P.nt + (size_t)t0 + l] / 8u;
            c.slot_reads += lds_read_cycles(s);
        }
        for (int r = 0; r < P.rpt; ++r) {
            for (int l = 0; l < 32; ++l) s[l] = P.oi[(size_t)r * P.nt + (size_t)t0 + l] / 8u;
            c.owner_reads += lds_read_cycles(s);
        }
    }
    return c;
}

}  // namespace ovqe
