// sparse_plan.hpp — the host's planner for the LDS traffic of the support-compacted kernels (sv_sparse.hpp): the compact numbering
// of the support, the rows of 32 lanes that k_sparse_vqe_rows / k_sparse_vqe_rows_shared walk, and the bank model both are chosen on.
//
// Pure host code on plain vectors (no HIP): tests/test_sparse_plan.py compiles it into a host program.  Everything is a function
// of the program alone (fixed seed, no clock): tables and energies stay reproducible.
//
// THE MODEL (lds_access_cycles).  An LDS access of a half-wave is served in aligned groups of lanes, one array cycle per group when
// no two lanes of the group want different words of one bank; every further distinct word on a busy bank adds a cycle; lanes with
// the same word share it.  For the 8-byte accesses of these kernels: a read is one group of 32 lanes against 32 banks (bank = slot
// mod 32), a write two groups of 16 contiguous lanes against 16 banks (bank = slot mod 16).  A shift of all slots by the same
// amount (the next state of a workgroup, SSTRIDE) permutes the banks and changes nothing.
//
// WHAT THE PLANNER MAY CHOOSE, and what each choice is worth:
//   * the residue mod 32 of every support element (plan_numbering);
//   * the ORIENTATION of a pair: rotating (j, i) by -s is rotating (i, j) by s — the same two fma on exchanged operands, the
//     same bits.  With it a row of up to 32 pairs reads conflict-free on both sides as soon as no residue holds more than TWO of
//     its 2 n elements: the elements with the pair edges and one "twin" edge per doubly used residue form paths and even cycles,
//     which two sides colour.  That is the condition the numbering search drives to zero — half as strict as one element per
//     residue and side, which the search could not reach (H2O: 2 of 308 accesses were conflict-free);
//   * the lane of a pair inside its row: with distinct residues mod 32 on a side at most two slots share a write bank (mod 16);
//     twins on the first and on the second index again form paths and even cycles, so the two halves of 16 lanes separate them;
//   * the spare slots of the padded lanes: a pad takes a spare slot whose read bank no lane of its row uses (one always exists:
//     at most 32 - pads banks are taken) and, among those, one whose write bank is free in its group of 16 where there is one.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace ovqe {

// LDS array cycles of ONE access of `nlanes` lanes (<= 64) to the 8-byte words slot[lane], served in aligned groups of `group`
// lanes against `banks` banks (<= 64): per group the largest number of distinct slots on one bank.
inline int lds_access_cycles(const uint32_t *slot, int nlanes, int group, int banks) {
    int cycles = 0;
    for (int g0 = 0; g0 < nlanes; g0 += group) {
        const int gn = std::min(group, nlanes - g0);
        uint32_t s[64];
        int cnt[64] = {};
        std::copy(slot + g0, slot + g0 + gn, s);
        std::sort(s, s + gn);
        const int nu = (int)(std::unique(s, s + gn) - s);
        int worst = 0;
        for (int k = 0; k < nu; ++k) worst = std::max(worst, ++cnt[s[k] % (uint32_t)banks]);
        cycles += worst;
    }
    return cycles;
}
inline int lds_read_cycles(const uint32_t *slot32) { return lds_access_cycles(slot32, 32, 32, 32); }     // ds_read_b64, one state
inline int lds_write_cycles(const uint32_t *slot32) { return lds_access_cycles(slot32, 32, 16, 16); }    // ds_write_b64

// pair word (sv_sparse.hpp): ci (12 bits) | cj (12 bits) << 12 | sign << 24 | pattern << 25
inline uint32_t pair_i(uint32_t pw) { return pw & 0xfffu; }
inline uint32_t pair_j(uint32_t pw) { return (pw >> 12) & 0xfffu; }

struct PlanOp { int32_t first, npairs; };   // the pairs of one op: disjoint

// one lane of a row of 32
struct RowLane {
    uint32_t si, sj;    // the slots the lane rotates, in the order the kernel takes them
    int32_t pair;       // index of the pair word (in the planned order); -1: a padded lane on two spare slots (identity entry)
    uint32_t swapped;   // 1: (si, sj) = (cj, ci) of the program's pair: the sign of its sine is flipped (SparsePlan::pairs has both)
};

struct RowCycles { int64_t reads = 0, writes = 0; };   // per evaluation: array cycles of the reads of i and j, of the writes of i and j

inline RowCycles rows_cycles(const std::vector<RowLane> &rows) {
    RowCycles c;
    for (size_t r0 = 0; r0 + 32 <= rows.size(); r0 += 32) {
        uint32_t a[32], b[32];
        for (int l = 0; l < 32; ++l) {
            a[l] = rows[r0 + l].si;
            b[l] = rows[r0 + l].sj;
        }
        c.reads += lds_read_cycles(a) + lds_read_cycles(b);
        c.writes += lds_write_cycles(a) + lds_write_cycles(b);
    }
    return c;
}

// colliding lane pairs per evaluation on the read side (ovqe_program_info [26..27]): per op and side, n elements on a residue mod 32
// where the op's chunks of 32 lanes hold `cap` count (n - cap)(n - cap + 1) / 2.  `swapped` (may be null): the orientation in use.
inline int64_t colliding_lane_pairs(const std::vector<PlanOp> &ops, const std::vector<uint32_t> &pairs, const std::vector<uint8_t> *swapped) {
    int64_t cost = 0;
    for (const PlanOp &op : ops) {
        int hist[2][32] = {};
        const int cap = (op.npairs + 31) / 32;
        for (int k = 0; k < op.npairs; ++k) {
            const uint32_t pw = pairs[(size_t)op.first + k];
            const int sw = swapped ? (*swapped)[(size_t)op.first + k] : 0;
            ++hist[sw][pair_i(pw) & 31u];
            ++hist[sw ^ 1][pair_j(pw) & 31u];
        }
        for (int s = 0; s < 2; ++s)
            for (int r = 0; r < 32; ++r)
                if (hist[s][r] > cap) cost += (int64_t)(hist[s][r] - cap) * (hist[s][r] - cap + 1) / 2;
    }
    return cost;
}

// ---- the numbering: slot[k] of support element k (discovery order), slots < *mp = 32 ceil(m / 32) ---------------------------------
// Residues mod 32 by a deterministic annealed local search (swap the residues of two elements, or move one into a class with room).
// The cost is the modelled excess of the rows' accesses over conflict-free ones once orientation, halves and pads are chosen as
// below: per op with c chunks, the elements (of both sides) on one residue beyond 2 c — each of them is a lane that some read of
// the op serves in an extra cycle, and no arrangement of the op can avoid it; at zero every read of a row costs one cycle and,
// with the halves, every write group one (a store's array cycles cost time only beyond the instruction's own transfer: nothing is
// left to charge).  Beyond 2 c the excess counts quadratically, as the pair count did: a residue three over is worse than three
// residues one over, which orientation spreads over two sides.  The budget depends on the program alone.
inline void plan_numbering(int m, const std::vector<PlanOp> &ops, const std::vector<uint32_t> &pairs, std::vector<int> *slot, int *mp) {
    const int nh = (int)ops.size();
    const int rows = (m + 31) / 32;
    std::vector<uint16_t> hist((size_t)nh * 32, 0);
    std::vector<int> cap((size_t)nh);
    std::vector<std::vector<int>> inc((size_t)m);
    for (int o = 0; o < nh; ++o) {
        cap[o] = 2 * ((ops[o].npairs + 31) / 32);
        for (int k = 0; k < ops[o].npairs; ++k) {
            const uint32_t pw = pairs[(size_t)ops[o].first + k];
            inc[pair_i(pw)].push_back(o);
            inc[pair_j(pw)].push_back(o);
        }
    }
    std::vector<int> res((size_t)m), count(32, 0);
    for (int k = 0; k < m; ++k) {
        res[k] = k & 31;
        ++count[k & 31];
        for (int o : inc[k]) ++hist[(size_t)o * 32 + (k & 31)];
    }
    auto excess = [](int n, int c) { return n > c ? (int64_t)(n - c) * (n - c + 1) / 2 : (int64_t)0; };
    int64_t cost = 0;
    for (int o = 0; o < nh; ++o)
        for (int r = 0; r < 32; ++r) cost += excess(hist[(size_t)o * 32 + r], cap[o]);
    auto move = [&](int e, int to) {   // -> change of the cost
        const int from = res[e];
        int64_t d = 0;
        for (int o : inc[e]) {
            uint16_t *hh = &hist[(size_t)o * 32];
            d += excess(hh[from] - 1, cap[o]) - excess(hh[from], cap[o]) + excess(hh[to] + 1, cap[o]) - excess(hh[to], cap[o]);
            --hh[from];
            ++hh[to];
        }
        res[e] = to;
        return d;
    };
    size_t total_inc = 0;
    for (const auto &v : inc) total_inc += v.size();
    const double avg_inc = std::max(1.0, (double)total_inc / m);
    const int64_t proposals = cost ? (int64_t)std::min(400.0 * m, 6e7 / avg_inc) : 0;
    uint64_t rng = 0x9e3779b97f4a7c15ull;
    auto next = [&]() {
        rng ^= rng << 13;
        rng ^= rng >> 7;
        rng ^= rng << 17;
        return rng;
    };
    for (int64_t it = 0; it < proposals && cost > 0; ++it) {
        const double temp = 0.6 * (1.0 - (double)it / (double)proposals) + 0.02;
        const int a = (int)(next() % (uint64_t)m);
        int64_t d;
        int b = -1, ra = res[a], rb;
        if ((next() & 3u) == 0) {                       // move into a residue class with a free slot
            rb = (int)(next() & 31u);
            if (rb == ra || count[rb] >= rows) continue;
            d = move(a, rb);
        } else {                                        // swap residues with another element
            b = (int)(next() % (uint64_t)m);
            rb = res[b];
            if (rb == ra) continue;
            d = move(a, rb);
            d += move(b, ra);
        }
        const bool accept = d <= 0 || (double)(next() >> 11) * (1.0 / 9007199254740992.0) < std::exp(-(double)d / temp);
        if (accept) {
            cost += d;
            if (b < 0) {
                --count[ra];
                ++count[rb];
            }
        } else {
            move(a, ra);
            if (b >= 0) move(b, rb);
        }
    }
    // slots: residue + 32 * (rank inside the residue class, by discovery order)
    slot->assign((size_t)m, 0);
    std::vector<int> fill(32, 0);
    for (int k = 0; k < m; ++k) (*slot)[k] = res[k] + 32 * fill[res[k]]++;
    *mp = 32 * rows;
}

// ---- rows in the order of the pair list, padded lanes l on the spare slots mp + l and mp + 32 + l ----------------------------------
// (what "sparse_renumber" = 0 runs, and what the figures for discovery order are taken on)
inline void plain_rows(const std::vector<PlanOp> &ops, const std::vector<uint32_t> &pairs, int mp, std::vector<RowLane> *rows) {
    rows->clear();
    for (const PlanOp &op : ops)
        for (int c0 = 0; c0 < op.npairs; c0 += 32)
            for (int lane = 0; lane < 32; ++lane) {
                if (c0 + lane >= op.npairs) {
                    rows->push_back({(uint32_t)(mp + lane), (uint32_t)(mp + 32 + lane), -1, 0u});
                    continue;
                }
                const uint32_t pw = pairs[(size_t)op.first + c0 + lane];
                rows->push_back({pair_i(pw), pair_j(pw), op.first + c0 + lane, 0u});
            }
}

// ---- planned rows: chunks, orientation, halves, pads -----------------------------------------------------------------------------
// pairs: slots already renumbered.  -> *rows (32 lanes per row, the rows of an op in a block, ops in order), *ordered: the pair
// words in the order of their lanes (each op a permutation of its own range; RowLane::pair indexes it), *swapped: per ordered word.
inline void plan_rows(const std::vector<PlanOp> &ops, const std::vector<uint32_t> &pairs, int mp, std::vector<RowLane> *rows,
                      std::vector<uint32_t> *ordered, std::vector<uint8_t> *swapped) {
    rows->clear();
    ordered->assign(pairs.size(), 0u);
    swapped->assign(pairs.size(), 0);
    struct Item { uint32_t pw, s[2]; };   // s[0] / s[1]: first / second slot as oriented
    for (const PlanOp &op : ops) {
        const int n = op.npairs, nch = (n + 31) / 32;
        // chunks of at most 32 pairs: a pair goes where its two residues are held by fewer than two elements so far, the emptier
        // chunk first (one chunk: all of them)
        std::vector<std::vector<uint32_t>> chunk((size_t)nch);
        if (nch == 1) {
            chunk[0].assign(pairs.begin() + op.first, pairs.begin() + op.first + n);
        } else {
            std::vector<int> cnt((size_t)nch * 32, 0);
            for (int k = 0; k < n; ++k) {
                const uint32_t pw = pairs[(size_t)op.first + k], ra = pair_i(pw) & 31u, rb = pair_j(pw) & 31u;
                int best = -1, best_over = 0;
                for (int c = 0; c < nch; ++c) {
                    if (chunk[c].size() >= 32) continue;
                    const int *cc = &cnt[(size_t)c * 32];
                    const int over = ra == rb ? (cc[ra] >= 1) : (cc[ra] >= 2) + (cc[rb] >= 2);
                    if (best < 0 || over < best_over || (over == best_over && chunk[c].size() < chunk[best].size())) {
                        best = c;
                        best_over = over;
                    }
                }
                chunk[best].push_back(pw);
                ++cnt[(size_t)best * 32 + ra];
                ++cnt[(size_t)best * 32 + rb];
            }
            // ... then pairs on a residue that holds more than two move to another chunk, or change places with a pair there,
            // as long as that lowers the elements beyond two of the two chunks together
            auto over2 = [&](int c) {
                int v = 0;
                for (int r = 0; r < 32; ++r) v += std::max(0, cnt[(size_t)c * 32 + r] - 2);
                return v;
            };
            auto count = [&](int c, uint32_t pw, int d) {
                cnt[(size_t)c * 32 + (pair_i(pw) & 31u)] += d;
                cnt[(size_t)c * 32 + (pair_j(pw) & 31u)] += d;
            };
            for (int pass = 0, moved = 1; moved && pass < 64; ++pass) {
                moved = 0;
                for (int c = 0; c < nch; ++c)
                    for (size_t a = 0; a < chunk[c].size(); ++a) {
                        const uint32_t pw = chunk[c][a];
                        if (cnt[(size_t)c * 32 + (pair_i(pw) & 31u)] <= 2 && cnt[(size_t)c * 32 + (pair_j(pw) & 31u)] <= 2) continue;
                        bool done = false;
                        for (int c2 = 0; c2 < nch && !done; ++c2) {
                            if (c2 == c) continue;
                            const int before = over2(c) + over2(c2);
                            count(c, pw, -1);
                            count(c2, pw, 1);
                            if (chunk[c2].size() < 32 && over2(c) + over2(c2) < before) {
                                chunk[c2].push_back(pw);
                                chunk[c].erase(chunk[c].begin() + (long)a);
                                done = true;
                                break;
                            }
                            for (size_t b = 0; b < chunk[c2].size() && !done; ++b) {
                                const uint32_t qw = chunk[c2][b];
                                count(c2, qw, -1);
                                count(c, qw, 1);
                                if (over2(c) + over2(c2) < before) {
                                    std::swap(chunk[c][a], chunk[c2][b]);
                                    done = true;
                                } else {
                                    count(c2, qw, 1);
                                    count(c, qw, -1);
                                }
                            }
                            if (!done) {
                                count(c, pw, 1);
                                count(c2, pw, -1);
                            }
                        }
                        if (done) {
                            moved = 1;
                            --a;   // (the pair now at this place is looked at next; unsigned wrap at 0)
                        }
                    }
            }
        }
        int at = op.first;
        for (int c = 0; c < nch; ++c) {
            const int cn = (int)chunk[c].size();
            std::vector<Item> it((size_t)cn);
            for (int t = 0; t < cn; ++t) it[t] = {chunk[c][t], {pair_i(chunk[c][t]), pair_j(chunk[c][t])}};
            // -- orientation: elements e = 2 t + (position in the word); the two elements of a pair take different sides, and so do
            // two elements (of different pairs) that share a residue — matched two by two where a residue holds more
            std::vector<int> twin((size_t)2 * cn, -1), side((size_t)2 * cn, -1), stack;
            {
                std::vector<int> by_res[32];
                for (int e = 0; e < 2 * cn; ++e) by_res[it[e >> 1].s[e & 1] & 31u].push_back(e);
                for (auto &lst : by_res) {
                    // (both elements of one pair on a residue are on different sides anyway: they do not take part)
                    std::vector<int> free_e;
                    for (int e : lst) {
                        bool own = false;
                        for (int f : lst) own |= f == (e ^ 1);
                        if (!own) free_e.push_back(e);
                    }
                    for (size_t q = 0; q + 1 < free_e.size(); q += 2) {
                        twin[free_e[q]] = free_e[q + 1];
                        twin[free_e[q + 1]] = free_e[q];
                    }
                }
            }
            for (int e0 = 0; e0 < 2 * cn; ++e0) {
                if (side[e0] >= 0) continue;
                side[e0] = e0 & 1;   // a free component keeps the orientation of the pair list
                stack.assign(1, e0);
                while (!stack.empty()) {
                    const int e = stack.back();
                    stack.pop_back();
                    const int nb[2] = {e ^ 1, twin[e]};
                    for (int f : nb)
                        if (f >= 0 && side[f] < 0) {
                            side[f] = side[e] ^ 1;
                            stack.push_back(f);
                        }
                }
            }
            std::vector<uint8_t> sw((size_t)cn, 0);
            for (int t = 0; t < cn; ++t)
                if (side[2 * t] == 1) {
                    sw[t] = 1;
                    std::swap(it[t].s[0], it[t].s[1]);
                }
            // -- halves of 16 lanes: pairs whose first slots, or whose second slots, are equal mod 16 go to different halves (matched
            // two by two); the components are then turned so that neither half exceeds 16
            std::vector<int> tw[2] = {std::vector<int>((size_t)cn, -1), std::vector<int>((size_t)cn, -1)}, col((size_t)cn, -1), comp((size_t)cn, -1);
            for (int s = 0; s < 2; ++s) {
                std::vector<int> by16[16];
                for (int t = 0; t < cn; ++t) by16[it[t].s[s] & 15u].push_back(t);
                for (auto &lst : by16)
                    for (size_t q = 0; q + 1 < lst.size(); q += 2) {
                        tw[s][lst[q]] = lst[q + 1];
                        tw[s][lst[q + 1]] = lst[q];
                    }
            }
            std::vector<int> c0s, c1s;   // per component: members of colour 0 / 1
            for (int t0 = 0; t0 < cn; ++t0) {
                if (col[t0] >= 0) continue;
                const int id = (int)c0s.size();
                c0s.push_back(0);
                c1s.push_back(0);
                col[t0] = 0;
                stack.assign(1, t0);
                while (!stack.empty()) {
                    const int t = stack.back();
                    stack.pop_back();
                    comp[t] = id;
                    ++(col[t] ? c1s : c0s)[id];
                    const int nb[2] = {tw[0][t], tw[1][t]};
                    for (int f : nb)
                        if (f >= 0 && col[f] < 0) {
                            col[f] = col[t] ^ 1;
                            stack.push_back(f);
                        }
                }
            }
            const int ncomp = (int)c0s.size();
            // reach[k][s]: the first k components can put s pairs into half 0; flip[k][s]: ... with component k - 1 turned
            std::vector<std::vector<int8_t>> reach((size_t)ncomp + 1, std::vector<int8_t>(33, -1));
            reach[0][0] = 0;
            for (int k = 0; k < ncomp; ++k)
                for (int s = 0; s <= 32; ++s) {
                    if (reach[k][s] < 0) continue;
                    if (s + c0s[k] <= 32 && reach[k + 1][s + c0s[k]] < 0) reach[k + 1][s + c0s[k]] = 0;
                    if (s + c1s[k] <= 32 && reach[k + 1][s + c1s[k]] < 0) reach[k + 1][s + c1s[k]] = 1;
                }
            int want = -1;
            for (int d = 0; d <= 32 && want < 0; ++d)   // as even as the components allow
                for (int s : {(cn + 1) / 2 + d, (cn + 1) / 2 - d})
                    if (want < 0 && s >= 0 && s <= 32 && reach[ncomp][s] >= 0) want = s;
            std::vector<int8_t> turned((size_t)ncomp, 0);
            for (int k = ncomp, s = want; k > 0; --k) {
                turned[k - 1] = reach[k][s];
                s -= turned[k - 1] ? c1s[k - 1] : c0s[k - 1];
            }
            std::vector<int> half[2];
            for (int t = 0; t < cn; ++t) half[col[t] ^ turned[comp[t]]].push_back(t);
            for (int hs = 0; hs < 2; ++hs)   // (no even split within 16: the overflow goes over)
                while (half[hs].size() > 16) {
                    half[hs ^ 1].push_back(half[hs].back());
                    half[hs].pop_back();
                }
            // -- lanes and pads
            RowLane row[32];
            uint32_t used32[2] = {0, 0}, used16[2][2] = {{0, 0}, {0, 0}}, spare_taken[2] = {0, 0};
            bool is_pad[32];
            for (int l = 0; l < 32; ++l) is_pad[l] = true;
            for (int hs = 0; hs < 2; ++hs)
                for (size_t q = 0; q < half[hs].size(); ++q) {
                    const int l = 16 * hs + (int)q, t = half[hs][q];
                    is_pad[l] = false;
                    row[l] = {it[t].s[0], it[t].s[1], 0, sw[t]};
                    for (int s = 0; s < 2; ++s) {
                        used32[s] |= 1u << (it[t].s[s] & 31u);
                        used16[hs][s] |= 1u << (it[t].s[s] & 15u);
                    }
                }
            for (int l = 0; l < 32; ++l) {   // the pair words in lane order
                if (is_pad[l]) continue;
                const int t = half[l >> 4][(size_t)(l & 15)];
                (*ordered)[(size_t)at] = it[t].pw;
                (*swapped)[(size_t)at] = sw[t];
                row[l].pair = at++;
            }
            for (int l = 0; l < 32; ++l) {
                if (!is_pad[l]) continue;
                uint32_t s2[2];
                for (int s = 0; s < 2; ++s) {
                    const uint32_t base = (uint32_t)mp + 32u * (uint32_t)s;
                    int pick = -1, grade = 0;   // 3: read and write bank free, 2: read bank free, 1: an unused spare
                    for (int q = 0; q < 32; ++q) {
                        if ((spare_taken[s] >> q) & 1u) continue;
                        const uint32_t sl = base + (uint32_t)q;
                        const int g = !((used32[s] >> (sl & 31u)) & 1u) ? (!((used16[l >> 4][s] >> (sl & 15u)) & 1u) ? 3 : 2) : 1;
                        if (g > grade) {
                            grade = g;
                            pick = q;
                        }
                    }
                    spare_taken[s] |= 1u << pick;
                    s2[s] = base + (uint32_t)pick;
                    used32[s] |= 1u << (s2[s] & 31u);
                    used16[l >> 4][s] |= 1u << (s2[s] & 15u);
                }
                row[l] = {s2[0], s2[1], -1, 0u};
            }
            rows->insert(rows->end(), row, row + 32);
        }
    }
}

// ---- the whole plan of a program ----------------------------------------------------------------------------------------------------
struct SparsePlan {
    int mp = 0;                       // slots of the support (renumbered: a multiple of 32); the spare slots follow
    std::vector<int> slot;            // support element (discovery order) -> slot
    std::vector<uint32_t> pairs;      // the pair words on slots, each op's in the order of their lanes, as oriented
    std::vector<uint8_t> swapped;     // per pair word: it is (cj, ci) of the program's pair, with the sign bit flipped
    std::vector<RowLane> rows;        // the rows of 32 in use
    int64_t conflicts_discovery = 0, conflicts = 0;   // colliding_lane_pairs in discovery order / as planned
    RowCycles cycles, cycles_discovery;               // modelled array cycles of the rows in use / of plain rows in discovery order
};

// pairs: on support elements in discovery order (0 .. m - 1 < 4096).  renumber = false: discovery order, plain rows.
inline void plan_sparse_program(int m, const std::vector<PlanOp> &ops, const std::vector<uint32_t> &pairs, bool renumber, SparsePlan *P) {
    P->slot.resize((size_t)m);
    for (int k = 0; k < m; ++k) P->slot[k] = k;
    P->mp = m;
    P->pairs = pairs;
    P->swapped.assign(pairs.size(), 0);
    plain_rows(ops, pairs, m, &P->rows);
    P->cycles = P->cycles_discovery = rows_cycles(P->rows);
    P->conflicts = P->conflicts_discovery = 0;
    if (!renumber || m <= 32 || m > 4064 || ops.empty()) return;
    P->conflicts_discovery = colliding_lane_pairs(ops, pairs, nullptr);
    plan_numbering(m, ops, pairs, &P->slot, &P->mp);
    std::vector<uint32_t> on_slots(pairs);
    for (uint32_t &pw : on_slots)
        pw = (pw & ~0xffffffu) | (uint32_t)P->slot[pair_i(pw)] | ((uint32_t)P->slot[pair_j(pw)] << 12);
    plan_rows(ops, on_slots, P->mp, &P->rows, &P->pairs, &P->swapped);
    P->cycles = rows_cycles(P->rows);
    P->conflicts = colliding_lane_pairs(ops, P->pairs, &P->swapped);
    // the orientation goes into the pair words: every kernel that walks them, or rows built from them, turns (cj, ci) by -s
    for (size_t k = 0; k < P->pairs.size(); ++k)
        if (P->swapped[k]) {
            const uint32_t pw = P->pairs[k];
            P->pairs[k] = ((pw & ~0x1ffffffu) | pair_j(pw) | (pair_i(pw) << 12) | (pw & (1u << 24))) ^ (1u << 24);
        }
}

// ---- the entry stream of the per-wave kernels -------------------------------------------------------------------------------------
// A wave reads the two amplitudes of 64 consecutive entries at once (two groups of 32 lanes).  The entries are a plain sum, so their
// order is free: they are re-arranged greedily so that inside every aligned group of 32 the first indices are distinct mod 32 and
// so are the second ones — conflict-free reads wherever the entry set allows it (a fixed order: results stay reproducible).
// E: a record with the member ij = ci | cj << 12.
template <class E>
inline void arrange_entries(std::vector<E> &entries) {
    if (entries.size() <= 64) return;
    std::vector<std::vector<uint32_t>> by_bank(32);
    for (uint32_t e = 0; e < (uint32_t)entries.size(); ++e) by_bank[entries[e].ij & 31u].push_back(e);
    std::vector<E> arranged;
    arranged.reserve(entries.size());
    size_t left = entries.size();
    std::vector<uint32_t> order(32);
    while (left) {
        for (uint32_t b = 0; b < 32; ++b) order[b] = b;
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return by_bank[a].size() > by_bank[b].size(); });
        uint32_t used_j = 0;
        size_t taken = 0;
        for (uint32_t bi : order) {
            std::vector<uint32_t> &lst = by_bank[bi];
            if (lst.empty()) continue;
            size_t pick = lst.size();
            for (size_t k = lst.size(); k-- > 0;) {           // newest first: cheap erase
                const uint32_t bj = (entries[lst[k]].ij >> 12) & 31u;
                if (!((used_j >> bj) & 1u)) {
                    pick = k;
                    break;
                }
            }
            if (pick == lst.size()) continue;                 // every candidate collides on the second index
            used_j |= 1u << ((entries[lst[pick]].ij >> 12) & 31u);
            arranged.push_back(entries[lst[pick]]);
            lst.erase(lst.begin() + (long)pick);
            ++taken;
            --left;
        }
        if (taken == 0) {                                     // only colliding entries remain: take one anyway
            for (auto &lst : by_bank)
                if (!lst.empty()) {
                    arranged.push_back(entries[lst.back()]);
                    lst.pop_back();
                    --left;
                    break;
                }
        }
        // pad the group to 32 with whatever is left so that later groups stay aligned
        while (taken && taken < 32 && left) {
            bool any = false;
            for (auto &lst : by_bank)
                if (!lst.empty() && taken < 32) {
                    arranged.push_back(entries[lst.back()]);
                    lst.pop_back();
                    --left;
                    ++taken;
                    any = true;
                }
            if (!any) break;
        }
    }
    entries.swap(arranged);
}

}  // namespace ovqe
