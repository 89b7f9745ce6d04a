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

namespace ovqe {

struct OwnerPack {
    int nt = 0, rpt = 0, epr = 0;
    int pieces = 0;              // sum over the rows of ceil(load / EPR): the pieces that hold entries (<= nt * rpt)
    std::vector<uint16_t> oi;    // [rpt][nt]        byte offset of the piece's owner amplitude
    std::vector<uint16_t> oj;    // [rpt * epr][nt]  byte offset of the slot's other amplitude (padding: the owner's)
    std::vector<double> c;       // [rpt * epr][nt]  coefficient (padding and empty pieces: 0)
};

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
            // slots: per instruction (slot k of the group) other amplitudes that differ mod 32 where the pieces allow, one greedy pass
            std::vector<uint32_t> rest[32];
            for (int l = 0; l < 32; ++l) {
                const size_t t = (size_t)t0 + l;
                if (lane_piece[l] < 0) {   // empty piece: any valid slot, coefficients 0
                    const uint16_t off = (uint16_t)(((uint32_t)l % (uint32_t)nslots) * 8u);
                    out->oi[(size_t)r * nt + t] = off;
                    for (int k = 0; k < epr; ++k) out->oj[((size_t)r * epr + k) * nt + t] = off;
                    continue;
                }
                const Piece &p = pcs[(size_t)lane_piece[l]];
                out->oi[(size_t)r * nt + t] = (uint16_t)(p.owner * 8u);
                rest[l] = p.ent;
            }
            for (int k = 0; k < epr; ++k) {
                uint32_t used = 0;
                for (int l = 0; l < 32; ++l) {
                    if (lane_piece[l] < 0) continue;
                    const size_t at = ((size_t)r * epr + k) * nt + (size_t)t0 + l;
                    const uint32_t own = pcs[(size_t)lane_piece[l]].owner;
                    if (rest[l].empty()) {   // tail: the owner's amplitude with coefficient 0
                        out->oj[at] = (uint16_t)(own * 8u);
                        continue;
                    }
                    size_t pick = 0;
                    for (size_t q = 0; q < rest[l].size(); ++q) {
                        const uint32_t e = rest[l][q], o = si[e] == own ? sj[e] : si[e];
                        if (!((used >> (o & 31u)) & 1u)) {
                            pick = q;
                            break;
                        }
                    }
                    const uint32_t e = rest[l][pick], o = si[e] == own ? sj[e] : si[e];
                    used |= 1u << (o & 31u);
                    out->oj[at] = (uint16_t)(o * 8u);
                    out->c[at] = c[e];
                    rest[l].erase(rest[l].begin() + (long)pick);
                }
            }
        }
    return left == 0;
}

}  // namespace ovqe
