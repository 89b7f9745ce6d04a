"""The host planner of the support-compacted kernels (openvqe_amd/csrc/sparse_plan.hpp: numbering, rows of 32 lanes, bank model) and
the slot order of the owner pieces (sparse_pack.hpp) on the CPU.  Both headers are pure host code; they are compiled here into a
small host program that runs what build_sparse_program runs: plan_sparse_program, the entries renumbered and arranged, and
pack_owner_pieces for the instance's shape.

Programs: H2O and LiH (STO-3G UCCSD) rebuilt from the Pauli masks in the order build_sparse_program discovers the support, and
designed programs whose ops have 1, 15, 16, 17, 31, 32, 33, 64 and 65 pairs (every pad count, both sides of the 16- and 32-lane
boundaries).  Checked: every active pair in exactly one non-pad lane, pads on spare slots, distinct slots in a row, the rows applied
to a random state in numpy against the pair list (a sign lost in an orientation swap shows here), identical tables from two runs,
the reported cycles against an independent numpy count, and the modelled cycles against the tables of the planner before this one.

MODELLED CYCLES OF THE PLANNER BEFORE (PARENT below): its numbering search (pair excess on the read side), chunks, halves, pads on
spare slots mp + lane and the greedy slot pass of pack_owner_pieces, run on the same inputs by the same model function —
per evaluation (row reads, row writes, contraction reads = slots + owners):
    H2O  673 (2.19 per access, 308 accesses)  1275 (4.14 per write of two groups)  817 = 779 + 38 (2.43 per slot read, 1.19 per owner read)
    LiH  385 (2.01, 192)                        604 (3.15)                           327 = 314 + 13 (2.31, 1.63)
This planner, same inputs: H2O 360 / 659 / 468, LiH 196 / 387 / 207 (totals 0.54 and 0.60 of the above).

Planner time is printed, not asserted (the library creates no handle without a device; set_hamiltonian + set_ucc_program + first
energy_batch on the GPU host: H2O 49 -> 35 ms, LiH 21 -> 12 ms per handle, profiles/planner_banks/README.md)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.util import _parity64, cascade_geometry, compile_generators, pattern_excitation, y_rotation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NT = 256
PARENT = {"H2O": (673, 1275, 817), "LiH": (385, 604, 327)}   # (row reads, row writes, contraction reads): see the module docstring
SHAPE = {"H2O": (4, 10), "LiH": (1, 17)}                    # (rpt, epr) of the instance that holds the program (sparse_host.inc)

MAIN = r"""
#include "sparse_pack.hpp"
#include <chrono>
#include <cstdio>
// in: int32 m, nops, npairs, nent, nt, rpt, epr, renumber; int32 npairs_of_op[nops]; uint32 pairs[npairs]; uint32 eij[nent]; double ec[nent]
// out: int32 mp, nrows, packed, 0; int64 row reads, row writes, slot reads, owner reads, reads / writes in discovery order, colliding
// lane pairs, ... in discovery order, microseconds; int32 slot[m]; RowLane rows[32 nrows]; uint32 pairs[npairs]; uint8 swapped[npairs]
struct Ent { uint32_t ij; double c; };
int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    int32_t hd[8];
    if (!f || std::fread(hd, 4, 8, f) != 8) return 2;
    const size_t m = (size_t)hd[0], nops = (size_t)hd[1], npairs = (size_t)hd[2], nent = (size_t)hd[3];
    std::vector<int32_t> np(nops);
    std::vector<uint32_t> pairs(npairs), eij(nent);
    std::vector<double> ec(nent);
    if (std::fread(np.data(), 4, nops, f) != nops || std::fread(pairs.data(), 4, npairs, f) != npairs ||
        std::fread(eij.data(), 4, nent, f) != nent || std::fread(ec.data(), 8, nent, f) != nent) return 2;
    std::fclose(f);
    std::vector<ovqe::PlanOp> ops;
    int32_t first = 0;
    for (size_t o = 0; o < nops; ++o) {
        ops.push_back({first, np[o]});
        first += np[o];
    }
    const auto t0 = std::chrono::steady_clock::now();
    ovqe::SparsePlan P;
    ovqe::plan_sparse_program((int)m, ops, pairs, hd[7] != 0, &P);
    std::vector<Ent> ents(nent);
    for (size_t e = 0; e < nent; ++e)
        ents[e] = {(uint32_t)P.slot[eij[e] & 0xfffu] | ((uint32_t)P.slot[(eij[e] >> 12) & 0xfffu] << 12), ec[e]};
    ovqe::arrange_entries(ents);
    std::vector<uint32_t> ei(nent), ej(nent);
    std::vector<double> cc(nent);
    for (size_t e = 0; e < nent; ++e) {
        ei[e] = ents[e].ij & 0xfffu;
        ej[e] = (ents[e].ij >> 12) & 0xfffu;
        cc[e] = ents[e].c;
    }
    ovqe::OwnerPack K;
    const bool packed = nent > 0 && ovqe::pack_owner_pieces(ei, ej, cc, P.mp, hd[4], hd[5], hd[6], &K);
    const int64_t us = (int64_t)std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    ovqe::PackCycles pc;
    if (packed) pc = ovqe::pack_cycles(K);
    const int32_t h4[4] = {P.mp, (int32_t)(P.rows.size() / 32), packed ? 1 : 0, 0};
    const int64_t fig[9] = {P.cycles.reads, P.cycles.writes, pc.slot_reads, pc.owner_reads, P.cycles_discovery.reads,
                            P.cycles_discovery.writes, P.conflicts, P.conflicts_discovery, us};
    static_assert(sizeof(ovqe::RowLane) == 16, "four 32-bit fields");
    f = std::fopen(argv[2], "wb");
    if (!f) return 2;
    std::fwrite(h4, 4, 4, f);
    std::fwrite(fig, 8, 9, f);
    std::fwrite(P.slot.data(), 4, m, f);
    std::fwrite(P.rows.data(), 16, P.rows.size(), f);
    std::fwrite(P.pairs.data(), 4, npairs, f);
    std::fwrite(P.swapped.data(), 1, npairs, f);
    std::fclose(f);
    return 0;
}
"""


class Plan:
    pass


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("sparse_plan")
    src, exe = d / "main.cpp", d / "plan"
    src.write_text(MAIN)
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "openvqe_amd", "csrc"),
                           "-o", str(exe), str(src)])
    count = [0]

    def run(prog, rpt, epr, renumber=1):
        m, ops, pairs, ei, ej, ec = prog
        count[0] += 1
        fin, fout = d / f"in{count[0]}.bin", d / f"out{count[0]}.bin"
        with open(fin, "wb") as f:
            f.write(np.array([m, len(ops), len(pairs), len(ec), NT, rpt, epr, renumber], np.int32).tobytes())
            f.write(np.asarray(ops, np.int32).tobytes())
            f.write(np.ascontiguousarray(pairs[:, 2]).astype(np.uint32).tobytes())
            f.write((np.asarray(ei, np.uint32) | (np.asarray(ej, np.uint32) << 12)).tobytes())
            f.write(np.asarray(ec, np.float64).tobytes())
        subprocess.check_call([str(exe), str(fin), str(fout)])
        P = Plan()
        with open(fout, "rb") as f:
            P.mp, P.nrows, P.packed, _ = (int(v) for v in np.frombuffer(f.read(16), np.int32))
            fig = [int(v) for v in np.frombuffer(f.read(72), np.int64)]
            (P.reads, P.writes, P.slot_reads, P.owner_reads, P.reads_disc, P.writes_disc, P.conflicts, P.conflicts_disc, P.us) = fig
            P.slot = np.frombuffer(f.read(4 * m), np.int32)
            rows = np.frombuffer(f.read(16 * 32 * P.nrows), np.uint32).reshape(P.nrows, 32, 4)
            P.si, P.sj, P.swapped = rows[..., 0].astype(np.int64), rows[..., 1].astype(np.int64), rows[..., 3].astype(np.int64)
            P.pair = rows[..., 2].astype(np.int32).astype(np.int64)
            P.words = np.frombuffer(f.read(4 * len(pairs)), np.uint32)
            P.word_swapped = np.frombuffer(f.read(len(pairs)), np.uint8)
            assert f.read() == b""
        return P

    return run


# ---- programs -------------------------------------------------------------------------------------------------------------------
def discovery_program(hf_index, rx, rz, rc, rp, seed=0):
    """the ops and pairs of a rotation program on its support in DISCOVERY order, as build_sparse_program finds them: per run of
    rotations with one x mask, the pairs (i, i ^ x), i without the pivot bit, of the support so far on which the run's angle is not
    identically zero (tests/util.support_closure).  -> (support size, pairs per op, pairs [n][3]: ci, cj, the 32-bit pair word with a
    seeded sign bit and pattern id — the planner must carry both through)"""
    ident = {int(hf_index): 0}
    S = [int(hf_index)]
    ops, pairs = [], []
    r, R = 0, len(rx)
    while r < R:
        x = int(rx[r])
        e = r
        while e < R and int(rx[e]) == x:
            e += 1
        if x:
            pivot = 1 << (x.bit_length() - 1)
            seen, i0s = set(), []
            for a in S:
                i0 = a ^ x if a & pivot else a
                if i0 not in seen:
                    seen.add(i0)
                    i0s.append(i0)
            i0 = np.array(i0s, np.uint64)
            form = {}
            for t in range(r, e):
                z = int(rz[t])
                ny = bin(x & z).count("1")
                amp = float(rc[t]) * (1j ** (ny % 4)) * (1.0 - 2.0 * _parity64(i0 & np.uint64(z)))
                form[int(rp[t])] = form.get(int(rp[t]), 0.0) + amp
            active = np.zeros(len(i0s), bool)
            for v in form.values():
                active |= v != 0
            n = 0
            for a, act in zip(i0s, active):
                if not act:
                    continue
                for b in (a, a ^ x):
                    if b not in ident:
                        ident[b] = len(S)
                        S.append(b)
                pairs.append((ident[a], ident[a ^ x]))
                n += 1
            if n:
                ops.append(n)
        r = e
    pairs = np.array(pairs, np.int64).reshape(-1, 2)
    rng = np.random.default_rng(seed)
    words = pairs[:, 0] | (pairs[:, 1] << 12) | (rng.integers(0, 2, len(pairs)) << 24) | (rng.integers(0, 4, len(pairs)) << 25)
    return np.array(S, np.uint64), np.array(ops, np.int32), np.column_stack([pairs, words])


_MOLECULES = {}


def molecule(name):
    """(m, ops, pairs, ei, ej, ec): the UCCSD program and the restricted Hamiltonian's entries on the support in discovery order"""
    if name not in _MOLECULES:
        from openvqe_amd import chem, fermion
        from openvqe_amd.backend import compile_ucc_program
        from tests.test_sparse_pack import restricted_hamiltonian
        mol = chem.molecule(name)
        mol.rhf()
        ham, hf = mol.jw_hamiltonian(), mol.hf_init()
        gens = fermion.uccsd_generators(mol.nao, mol.n_elec // 2)
        n = ham.nbqbits
        rx, rz, rc, rp, _ = compile_ucc_program(n, gens)
        hf_index = int(sum(1 << (n - 1 - q) for q, v in enumerate(hf) if v)) if not np.isscalar(hf) else int(hf)
        S, ops, pairs = discovery_program(hf_index, rx, rz, rc, rp)
        m, si, sj, c = restricted_hamiltonian(name)       # on the SORTED support
        rank = {int(v): k for k, v in enumerate(S)}
        to_discovery = np.array([rank[int(v)] for v in np.sort(S)], np.uint32)
        assert m == S.size
        _MOLECULES[name] = (m, ops, pairs, to_discovery[si], to_discovery[sj], c)
    return _MOLECULES[name]


def designed_generators(s):
    """generators of a program with an op of exactly ``s`` pairs: a support of s basis states (tests/util.cascade_geometry: 2^k, or
    2^(k+1) - 1 with the single excitations, + 1 by an excitation that only the state with bits 1..k set takes), then Y rotations on fresh
    bits — the first has one pair per support state, each further one twice as many — until the register has 8 bits and the support
    more than 32 states (smaller ones are not renumbered).  s = 1: pairs 1, 2, 4, ..., 64.  -> (n_bits, hf_index, gens, K)"""
    if s == 1:
        n, hf, gens, K = 1, 1, [], 0
    elif s in (15, 31):
        k = {15: 3, 31: 4}[s]
        n, hf, gens, K = cascade_geometry(k, k, 0)
    else:
        k = {16: 4, 17: 4, 32: 5, 33: 5, 64: 6, 65: 6}[s]
        n, hf, gens, K = cascade_geometry(k, 0, 0)
        if s & 1:
            gens = gens + [pattern_excitation(list(range(1, k + 1)), [k + 1]) + (K,)]   # (2^k strings: an op holds at most 127)
            n, K = n + 1, K + 1
    size = s
    while size == s or n < 8 or size <= 32:
        gens = gens + [y_rotation(n) + (K,)]
        n, K, size = n + 1, K + 1, 2 * size
    return n, hf, gens, K


DESIGNED = [1, 15, 16, 17, 31, 32, 33, 64, 65]


def designed(s):
    n, hf, gens, K = designed_generators(s)
    rx, rz, rc, rp = compile_generators(gens)
    S, ops, pairs = discovery_program(hf, rx, rz, rc, rp, seed=s)
    assert s in ops.tolist(), (s, ops)
    m = S.size
    rng = np.random.default_rng(s)
    iu, ju = np.triu_indices(m)
    keep = (iu == ju) | (rng.random(iu.size) < min(1.0, 6.0 / m))
    return m, ops, pairs, iu[keep].astype(np.uint32), ju[keep].astype(np.uint32), rng.normal(size=int(keep.sum()))


# ---- the model, counted independently -------------------------------------------------------------------------------------------
def access_cycles(slots, group, banks):
    total = 0
    for g0 in range(0, len(slots), group):
        distinct = np.unique(slots[g0:g0 + group])
        total += int(np.bincount(distinct % banks, minlength=banks).max())
    return total


def _check_plan(P, prog, renumbered):
    m, ops, pairs = prog[0], prog[1], prog[2]
    nrows = int(sum(-(-int(n) // 32) for n in ops))
    assert P.nrows == nrows
    if renumbered:
        assert P.mp == 32 * -(-m // 32)
        assert np.unique(P.slot).size == m and P.slot.min() >= 0 and P.slot.max() < P.mp
    else:
        assert P.mp == m and np.array_equal(P.slot, np.arange(m))
    pad = P.pair < 0
    # every active pair in exactly one non-pad lane of a row of its own op, on its slots, and the pair word kept (sign bit, pattern)
    want_words = (P.slot[pairs[:, 0]] | (P.slot[pairs[:, 1]] << 12) | (pairs[:, 2] & ~0xFFFFFF)).astype(np.uint32)
    wi, wj = (P.words & 0xFFF).astype(np.int64), ((P.words >> 12) & 0xFFF).astype(np.int64)
    ws = P.word_swapped.astype(bool)
    # (an oriented word is (cj, ci) with the sign bit flipped)
    unoriented = np.where(ws, ((P.words & ~np.uint32(0x1FFFFFF)) | wj.astype(np.uint32) | (wi.astype(np.uint32) << 12)
                               | ((P.words ^ np.uint32(1 << 24)) & np.uint32(1 << 24))), P.words).astype(np.uint32)
    assert np.array_equal(np.sort(unoriented), np.sort(want_words))
    assert np.array_equal(np.sort(P.pair[~pad]), np.arange(len(pairs)))
    k = P.pair[~pad]
    assert np.array_equal(ws[k], P.swapped[~pad] == 1)
    assert np.array_equal(P.si[~pad], wi[k]) and np.array_equal(P.sj[~pad], wj[k])
    row, first = 0, 0
    for n in ops:
        nch = -(-int(n) // 32)
        lanes = P.pair[row:row + nch]
        assert np.array_equal(np.sort(lanes[lanes >= 0]), np.arange(first, first + n))
        # (the ordered words of an op are a permutation of the op's own)
        assert np.array_equal(np.sort(unoriented[first:first + n]), np.sort(want_words[first:first + n]))
        row, first = row + nch, first + int(n)
    # pads: an i-spare and a j-spare; slots distinct within a row
    assert ((P.si[pad] >= P.mp) & (P.si[pad] < P.mp + 32)).all() and ((P.sj[pad] >= P.mp + 32) & (P.sj[pad] < P.mp + 64)).all()
    assert (P.si[~pad] < P.mp).all() and (P.sj[~pad] < P.mp).all()
    both = np.concatenate([P.si, P.sj], axis=1)
    assert all(np.unique(r).size == 64 for r in both)
    # the reported cycles
    reads = sum(access_cycles(P.si[r], 32, 32) + access_cycles(P.sj[r], 32, 32) for r in range(nrows))
    writes = sum(access_cycles(P.si[r], 16, 16) + access_cycles(P.sj[r], 16, 16) for r in range(nrows))
    assert (reads, writes) == (P.reads, P.writes)
    assert reads >= 2 * nrows and writes >= 4 * nrows


def _apply_check(P, prog, seed):
    """the rows on a random state against the pair list in its own order and orientation: bit for bit"""
    m, ops, pairs = prog[0], prog[1], prog[2]
    rng = np.random.default_rng(seed)
    angle = rng.uniform(-3, 3, (len(ops), 4))
    a0 = rng.normal(size=m)
    want = a0.copy()
    first = 0
    for o, n in enumerate(ops):
        for ci, cj, w in pairs[first:first + n]:
            c, s = np.cos(angle[o, (w >> 25) & 3]), np.sin(angle[o, (w >> 25) & 3]) * (-1.0 if (w >> 24) & 1 else 1.0)
            u, v = want[ci], want[cj]
            want[ci], want[cj] = c * u + s * v, c * v - s * u
        first += int(n)
    st = np.zeros(P.mp + 64)
    st[P.slot] = a0
    row = 0
    for o, n in enumerate(ops):
        for _ in range(-(-int(n) // 32)):
            si, sj, pr = P.si[row], P.sj[row], P.pair[row]
            w = np.where(pr >= 0, P.words[np.maximum(pr, 0)], 0).astype(np.int64)
            ang = angle[o, (w >> 25) & 3]
            c = np.where(pr >= 0, np.cos(ang), 1.0)
            s = np.where(pr >= 0, np.sin(ang) * np.where((w >> 24) & 1, -1.0, 1.0), 0.0)
            u, v = st[si], st[sj]              # (all lanes read, then all lanes write: the slots of a row are distinct)
            st[si], st[sj] = c * u + s * v, c * v - s * u
            row += 1
    assert np.array_equal(st[P.slot], want)
    assert not st[P.mp:].any()


# ---- tests ----------------------------------------------------------------------------------------------------------------------
def test_the_model_function_on_known_accesses(planner):
    """the numpy count used below, on accesses whose cycles are known: conflict-free, broadcast, n-way, groups of 16"""
    assert access_cycles(np.arange(32), 32, 32) == 1 and access_cycles(np.arange(32), 16, 16) == 2
    assert access_cycles(np.zeros(32, np.int64), 32, 32) == 1                      # one word
    assert access_cycles(np.arange(32) * 32, 32, 32) == 32                         # one bank
    assert access_cycles(np.arange(32) % 16 + 32 * (np.arange(32) // 16), 32, 32) == 2
    assert access_cycles(np.arange(32), 32, 32) + access_cycles(np.arange(32) * 2, 16, 16) == 1 + 4   # writes: slots 0 and 16 share a bank


@pytest.mark.parametrize("mol, support, nops, npairs, entries", [("H2O", 441, 140, 3620, 9443), ("LiH", 225, 92, 1548, 3243)])
def test_molecules(planner, mol, support, nops, npairs, entries):
    prog = molecule(mol)
    assert (prog[0], len(prog[1]), len(prog[2]), len(prog[5])) == (support, nops, npairs, entries)
    P = planner(prog, *SHAPE[mol])
    _check_plan(P, prog, True)
    _apply_check(P, prog, 7)
    assert P.packed
    # sp_conflicts keeps its meaning and its order (tests/test_gpu_kernels.py)
    assert 0 <= P.conflicts <= P.conflicts_disc
    # discovery order: what "sparse_renumber" = 0 runs
    D = planner(prog, *SHAPE[mol], renumber=0)
    _check_plan(D, prog, False)
    _apply_check(D, prog, 8)
    assert (D.reads, D.writes) == (P.reads_disc, P.writes_disc) == (D.reads_disc, D.writes_disc)
    assert not D.swapped.any() and not D.word_swapped.any() and D.conflicts == 0 == D.conflicts_disc
    # the model against the planner before
    p_reads, p_writes, p_h = PARENT[mol]
    h = P.slot_reads + P.owner_reads
    ratio = (P.reads + P.writes + h) / (p_reads + p_writes + p_h)
    print(f"{mol}: row reads {P.reads} ({p_reads}), row writes {P.writes} ({p_writes}), contraction {P.slot_reads} + {P.owner_reads} "
          f"({p_h}); total {ratio:.3f} of the planner before; discovery order {P.reads_disc} / {P.writes_disc}; {P.us / 1e3:.1f} ms")
    assert P.reads <= p_reads and P.writes <= p_writes and h <= p_h
    if mol == "H2O":
        assert ratio <= 0.75


@pytest.mark.parametrize("mol", ["H2O", "LiH"])
def test_tables_are_a_function_of_the_program(planner, mol):
    prog = molecule(mol)
    A, B = planner(prog, *SHAPE[mol]), planner(prog, *SHAPE[mol])
    for name in ("mp", "nrows", "reads", "writes", "slot_reads", "owner_reads", "conflicts"):
        assert getattr(A, name) == getattr(B, name)
    for name in ("slot", "si", "sj", "pair", "swapped", "words", "word_swapped"):
        assert np.array_equal(getattr(A, name), getattr(B, name))


@pytest.mark.parametrize("s", DESIGNED)
def test_designed_pair_counts(planner, s):
    prog = designed(s)
    assert prog[0] > 32
    for rpt, epr in ((1, 17), (4, 10)):
        P = planner(prog, rpt, epr)
        _check_plan(P, prog, True)
        _apply_check(P, prog, s)
        assert P.conflicts <= P.conflicts_disc
        assert P.reads <= P.reads_disc and P.writes <= P.writes_disc
    D = planner(prog, 4, 10, renumber=0)
    _check_plan(D, prog, False)
    _apply_check(D, prog, s + 100)
