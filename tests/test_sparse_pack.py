"""The owner-piece packer of the batched sparse kernel (openvqe_amd/csrc/sparse_pack.hpp: pack_owner_pieces) on the CPU.  The
header is pure host code; it is compiled here into a small host program (the library itself needs a device for every handle).

Inputs: the restricted Hamiltonians of H2O and LiH (STO-3G UCCSD: 441 and 225 amplitudes) computed here from the Pauli masks, a
diagonal-only set, a set with one very heavy row, seeded random symmetric sets and sets that cannot fit.  Checked on the packed
tables: every input entry exactly once and owned by one of its endpoints, one owner per piece, padding with c = 0 and offsets in
range, the piece count, and the quadratic form in numpy against a^T H a from the unpacked entries."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from openvqe_amd.operators import pack_terms
from tests.util import support_closure

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NT = 256   # threads of a workgroup of k_sparse_vqe_rows_shared<4, ...>

MAIN = r"""
#include "sparse_pack.hpp"
#include <cstdio>
// in: int32 nslots, nt, rpt, epr, n; uint32 si[n]; uint32 sj[n]; double c[n]
// out: int32 ok, pieces; uint16 oi[rpt * nt]; uint16 oj[rpt * epr * nt]; double c[rpt * epr * nt]
int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hd[5];
    if (std::fread(hd, 4, 5, f) != 5) return 2;
    const size_t n = (size_t)hd[4];
    std::vector<uint32_t> si(n), sj(n);
    std::vector<double> c(n);
    if (std::fread(si.data(), 4, n, f) != n || std::fread(sj.data(), 4, n, f) != n || std::fread(c.data(), 8, n, f) != n) return 2;
    std::fclose(f);
    ovqe::OwnerPack P;
    const int32_t res[2] = {ovqe::pack_owner_pieces(si, sj, c, hd[0], hd[1], hd[2], hd[3], &P) ? 1 : 0, P.pieces};
    f = std::fopen(argv[2], "wb");
    if (!f) return 2;
    std::fwrite(res, 4, 2, f);
    if (res[0]) {
        std::fwrite(P.oi.data(), 2, P.oi.size(), f);
        std::fwrite(P.oj.data(), 2, P.oj.size(), f);
        std::fwrite(P.c.data(), 8, P.c.size(), f);
    }
    std::fclose(f);
    return 0;
}
"""


@pytest.fixture(scope="module")
def packer(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("sparse_pack")
    src, exe = d / "main.cpp", d / "pack"
    src.write_text(MAIN)
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "openvqe_amd", "csrc"),
                           "-o", str(exe), str(src)])
    count = [0]

    def run(si, sj, c, nslots, rpt, epr, nt=NT):
        count[0] += 1
        fin, fout = d / f"in{count[0]}.bin", d / f"out{count[0]}.bin"
        with open(fin, "wb") as f:
            f.write(np.array([nslots, nt, rpt, epr, len(c)], np.int32).tobytes())
            f.write(np.asarray(si, np.uint32).tobytes())
            f.write(np.asarray(sj, np.uint32).tobytes())
            f.write(np.asarray(c, np.float64).tobytes())
        subprocess.check_call([str(exe), str(fin), str(fout)])
        with open(fout, "rb") as f:
            ok, pieces = np.frombuffer(f.read(8), np.int32)
            if not ok:
                return None
            oi = np.frombuffer(f.read(2 * rpt * nt), np.uint16).reshape(rpt, nt)
            oj = np.frombuffer(f.read(2 * rpt * epr * nt), np.uint16).reshape(rpt, epr, nt)
            cc = np.frombuffer(f.read(8 * rpt * epr * nt), np.float64).reshape(rpt, epr, nt)
        return int(pieces), oi, oj, cc

    return run


def _parity(v):
    v = v.copy()
    for s in (32, 16, 8, 4, 2, 1):
        v ^= v >> np.uint64(s)
    return (v & np.uint64(1)).astype(np.int64)


def restricted_hamiltonian(mol_name):
    """(slot i, slot j, c) of sum c a_i a_j = <psi|H|psi> on the support of the molecule's UCCSD program: c = H_ii, or 2 H_ij with
    the pair counted once (what build_sparse_program forms).  <a ^ x| P |a> = i^ny (-1)^popcount(a & z), real amplitudes: even ny."""
    from openvqe_amd import chem, fermion
    from openvqe_amd.backend import compile_ucc_program
    mol = chem.molecule(mol_name)
    mol.rhf()
    ham, hf = mol.jw_hamiltonian(), mol.hf_init()
    gens = fermion.uccsd_generators(mol.nao, mol.n_elec // 2)
    n = ham.nbqbits
    rx, rz, rc, rp, _ = compile_ucc_program(n, gens)
    hf_index = int(sum(1 << (n - 1 - q) for q, v in enumerate(hf) if v)) if not np.isscalar(hf) else int(hf)
    S = support_closure(hf_index, rx, rz, rc, rp)
    hx, hz, hc = pack_terms(n, ham.terms)
    si, sj, cs = [], [], []
    for x in np.unique(hx):
        sel = hx == x
        pivot = np.uint64(1 << (int(x).bit_length() - 1)) if x else np.uint64(0)
        a = S[(S & pivot) == 0] if x else S
        b = a ^ x
        pos = np.searchsorted(S, b)
        inside = (pos < S.size) & (S[np.minimum(pos, S.size - 1)] == b)
        a, b, pos = a[inside], b[inside], pos[inside]
        d = np.zeros(a.size)
        for z, c in zip(hz[sel], hc[sel]):
            ny = bin(int(x) & int(z)).count("1")
            if ny & 1:
                continue
            d += (c * 1j ** ny).real * (1 - 2 * _parity(a & z))
        keep = d != 0
        si += np.searchsorted(S, a[keep]).tolist()
        sj += pos[keep].tolist()
        cs += ((2.0 if x else 1.0) * d[keep]).tolist()
    return S.size, np.array(si, np.uint32), np.array(sj, np.uint32), np.array(cs)


def _check(packed, si, sj, c, nslots, rpt, epr, nt=NT, seed=0):
    pieces, oi, oj, cc = packed
    assert (oi % 8 == 0).all() and (oj % 8 == 0).all()
    pi, pj = oi.astype(np.int64) // 8, oj.astype(np.int64) // 8
    assert pi.max() < nslots and pj.max() < nslots            # padding and empty pieces included
    # every input entry exactly once (as the unordered pair it is), owned by one of its endpoints; everything else is padding
    real = cc != 0
    own = np.broadcast_to(pi[:, None, :], pj.shape)
    key_in = np.minimum(si, sj).astype(np.int64) * nslots + np.maximum(si, sj)
    assert np.unique(key_in).size == key_in.size
    nz = c != 0
    key_out = np.minimum(own, pj)[real] * nslots + np.maximum(own, pj)[real]
    order_in, order_out = np.argsort(key_in[nz]), np.argsort(key_out)
    assert np.array_equal(key_in[nz][order_in], key_out[order_out])
    assert np.array_equal(c[nz][order_in], cc[real][order_out])      # the coefficients bit for bit
    # padding: c = 0 (by construction of `real`); the tail of a piece reads its owner, an empty piece one slot
    used = real.any(axis=1)
    tail = ~real & np.broadcast_to(used[:, None, :], real.shape)
    zero_in = int((~nz).sum())                                    # (input entries with c = 0 may sit anywhere)
    assert (pj[tail] != own[tail]).sum() <= zero_in
    # one owner per piece holds by layout (one oi per piece); the count of pieces in use
    load = np.zeros(nslots, np.int64)
    np.add.at(load, own[:, 0, :][used], real.sum(axis=1)[used])
    row_pieces = np.zeros(nslots, np.int64)
    np.add.at(row_pieces, own[:, 0, :][used], 1)
    assert (row_pieces >= -(-load // epr)).all()
    assert (-(-load // epr)).sum() <= nt * rpt
    assert pieces <= nt * rpt and int(used.sum()) <= pieces
    # the quadratic form
    rng = np.random.default_rng(seed)
    bound = 1e-13 * max(np.abs(c).sum(), 1e-300)
    for _ in range(4):
        a = rng.normal(size=nslots)
        want = float(np.sum(c * a[si] * a[sj]))
        t = np.einsum("rkt,rkt->rt", cc, a[pj])
        got = float(np.sum(a[pi] * t))
        assert abs(got - want) <= bound, (got, want, bound)


# the shapes the library ships (sparse_host.inc: launch_rows_shared instances) and the other candidates that were measured
H2O_SHAPES = [(4, 10), (2, 24), (3, 13)]
LIH_SHAPES = [(1, 17), (2, 8), (2, 9)]


@pytest.mark.parametrize("mol, shapes, support, entries", [("H2O", H2O_SHAPES, 441, 9443), ("LiH", LIH_SHAPES, 225, 3243)])
def test_molecules(packer, mol, shapes, support, entries):
    m, si, sj, c = restricted_hamiltonian(mol)
    assert m == support and c.size == entries
    assert int((si == sj).sum()) == support
    for rpt, epr in shapes:
        packed = packer(si, sj, c, m, rpt, epr)
        assert packed is not None, (mol, rpt, epr)
        print(f"{mol} {rpt} x {epr}: {packed[0]} pieces of {NT * rpt}, {rpt * (epr + 1)} reads per thread and state")
        _check(packed, si, sj, c, m, rpt, epr)


def test_diagonal_only(packer):
    m = 300
    idx = np.arange(m, dtype=np.uint32)
    c = np.random.default_rng(1).normal(size=m)
    packed = packer(idx, idx, c, m, 2, 3)
    assert packed is not None and packed[0] == m
    _check(packed, idx, idx, c, m, 2, 3)
    assert packer(idx, idx, c, m, 1, 3) is None                # 300 rows, 256 pieces


def test_one_very_heavy_row(packer):
    """a star: slot 7 is coupled to every other slot (its row alone would take 50 pieces of 10) + a diagonal"""
    m = 500
    others = np.array([k for k in range(m) if k != 7], np.uint32)
    si = np.concatenate([np.full(m - 1, 7, np.uint32), np.arange(m, dtype=np.uint32)])
    sj = np.concatenate([others, np.arange(m, dtype=np.uint32)])
    c = np.random.default_rng(2).normal(size=si.size)
    for rpt, epr in ((2, 10), (4, 3)):
        packed = packer(si, sj, c, m, rpt, epr)
        assert packed is not None
        _check(packed, si, sj, c, m, rpt, epr)
    # ... and with the other endpoints in the first position
    packed = packer(sj, si, c, m, 2, 10)
    assert packed is not None
    _check(packed, sj, si, c, m, 2, 10)


@pytest.mark.parametrize("seed", range(8))
def test_random_symmetric_sets(packer, seed):
    rng = np.random.default_rng(1000 + seed)
    m = int(rng.integers(2, 600))
    density = rng.uniform(0.005, 0.08)
    iu, ju = np.triu_indices(m)
    keep = (rng.random(iu.size) < density) | ((iu == ju) & (rng.random(iu.size) < 0.7))
    si, sj = iu[keep].astype(np.uint32), ju[keep].astype(np.uint32)
    swap = rng.random(si.size) < 0.5
    si, sj = np.where(swap, sj, si), np.where(swap, si, sj)
    perm = rng.permutation(si.size)
    si, sj = si[perm], sj[perm]
    c = rng.normal(size=si.size)
    rpt, epr = int(rng.integers(1, 5)), int(rng.integers(1, 25))
    packed = packer(si, sj, c, m, rpt, epr)
    deg = np.bincount(np.concatenate([si, sj[si != sj]]), minlength=m)
    # whatever the owners, sum ceil(load / epr) < n / epr + (rows that own anything) <= n / epr + (slots with an entry): below the
    # capacity the packer must succeed; above the capacity in slots it must fail; between the two either answer is right
    if c.size / epr + int((deg > 0).sum()) <= NT * rpt:
        assert packed is not None, (m, c.size, rpt, epr)
    if c.size > NT * rpt * epr:
        assert packed is None
    if packed is not None:
        _check(packed, si, sj, c, m, rpt, epr, seed=seed)


def test_sets_that_cannot_fit_report_failure(packer):
    m = 400
    iu, ju = np.triu_indices(m)
    si, sj = iu.astype(np.uint32), ju.astype(np.uint32)            # dense: 80 200 entries
    c = np.ones(si.size)
    assert packer(si, sj, c, m, 4, 10) is None                   # 10 240 slots
    assert packer(si[:10241], sj[:10241], c[:10241], m, 4, 10) is None
    idx = np.arange(m, dtype=np.uint32)
    assert packer(idx, idx, np.ones(m), m, 1, 24) is None          # 400 owners, 256 pieces
    assert packer(idx, idx, np.ones(m), m - 1, 4, 10) is None      # a slot out of range
