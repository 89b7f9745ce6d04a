"""CPU tests of the subspace-expansion matrices (ovqe_subspace_matrices): the checker of tests/subspace_cases.py against dense
Kronecker operators, the new symbols in header / cdef / ctypes table, ``excited.solve`` on the checker's matrices against the exact
spectrum of small synthetic molecules, the excitation operators, and the host-side plan (openvqe_amd/csrc/sv_subspace_host.hpp)
replayed by tests/cpu/subspace_plan_check.cpp under ASan + UBSan with g++ alone."""
import os
import subprocess

import numpy as np
import pytest

from openvqe_amd import excited, fermion
from oracle import dense
from tests import subspace_cases as sc
from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n", [4, 6])
def test_checker_equals_dense_kronecker_operators(n):
    rng = np.random.default_rng(40 + n)
    psi = util.random_state(rng, n)
    ham = util.random_hamiltonian(rng, n, 12, constant=0.625)
    ops = sc.random_pool(rng, n, 7)
    S, G, rows = sc.matrices(psi, n, ops, ham)
    mats = [dense.operator_matrix(op, sparse=False) for op in ops]
    hmat = dense.operator_matrix(ham, sparse=False)
    Phi = np.array([M @ psi for M in mats])
    want_S = Phi.conj() @ Phi.T
    want_G = Phi.conj() @ (hmat @ Phi.T)
    assert np.abs(S - want_S).max() < 1e-13 and np.abs(G - want_G).max() < 1e-13
    assert np.abs(mats[0] - np.eye(1 << n)).max() == 0.0 and abs(S[0, 0] - 1.0) < 1e-13
    assert rows == 1 << n
    only_S, none, _ = sc.matrices(psi, n, ops, None)
    assert none is None and np.array_equal(only_S, S)


def test_checker_row_count_on_a_sparse_state():
    n = 6
    psi = np.zeros(1 << n, np.complex128)
    psi[[3, 40]] = [0.6, 0.8j]
    ops = [sc.identity(n), sc.Hamiltonian(n, [sc.Term(1.0, "X", [n - 1]), sc.Term(0.5j, "ZY", [0, n - 1])]), sc.Hamiltonian(n, [], 0.0)]
    S, _, rows = sc.matrices(psi, n, ops, None)
    assert rows == 4                      # {3, 40} and their partners under x = 1
    assert np.all(S[2] == 0) and np.all(S[:, 2] == 0)


def test_subspace_symbols_are_declared_everywhere():
    from openvqe_amd import _lib
    header = open(os.path.join(ROOT, "include", "ovqe_sv.h")).read()
    cdef = open(os.path.join(ROOT, "include", "ovqe_sv.cdef.h")).read()
    for name in ("ovqe_subspace_matrices", "ovqe_subspace_info"):
        assert name + "(" in header and name + "(" in cdef and name in _lib.SIGNATURES
    assert '"subspace_workspace_mb"' in header
    from openvqe_amd.backend import Statevector
    from openvqe_amd.partitioned import PartitionedStatevector
    for m in ("subspace_matrices", "subspace_info"):
        assert callable(getattr(Statevector, m))
    with pytest.raises(NotImplementedError):
        PartitionedStatevector.subspace_matrices(None, [])


# ---- excited.solve on the checker's matrices ------------------------------------------------------------------------------------------
def _solve_case(mol, deexcitations):
    ops = mol.pool(deexcitations)
    S, G, _ = sc.matrices(mol.psi, mol.n, ops, mol.ham)
    ratio = sc.assert_spectrum_gap(S)
    energies, y, rank = excited.solve(0.5 * (G + G.conj().T), S)
    assert rank == int((ratio > 1e-10).sum()) == energies.shape[0] == y.shape[1]
    assert np.abs(y.conj().T @ S @ y - np.eye(rank)).max() < 1e-9
    return ops, S, G, energies, rank


@pytest.fixture(scope="module")
def mol427():
    return sc.Molecule(4, 2, 7)


def test_solve_spans_the_whole_sector_of_two_orbitals():
    mol = sc.Molecule(2, 1, 3)
    ops, _, _, energies, rank = _solve_case(mol, False)
    assert len(ops) == 4 and mol.sector.shape[0] == 4 and rank == 4
    assert np.abs(energies - mol.block_energies).max() < 1e-9


def test_solve_with_deexcitations_spans_the_sector_of_three_orbitals():
    mol = sc.Molecule(3, 1, 5)
    ops, _, _, energies, rank = _solve_case(mol, True)
    assert len(ops) == 17 and mol.sector.shape[0] == 9 and rank == 9
    assert np.abs(energies - mol.block_energies).max() < 1e-9


def test_solve_interlaces_on_four_orbitals(mol427):
    ops, _, _, energies, rank = _solve_case(mol427, False)
    assert len(ops) == 27 and rank == 27 and mol427.sector.shape[0] == 36
    assert abs(energies[0] - mol427.block_energies[0]) < 1e-9
    assert np.all(energies >= mol427.block_energies[:27] - 1e-9)


def test_solve_drops_exactly_one_direction_for_an_operator_passed_twice(mol427):
    ops, _, _, energies, rank = _solve_case(mol427, False)
    twice = ops + [ops[5]]
    S, G, _ = sc.matrices(mol427.psi, mol427.n, twice, mol427.ham)
    sc.assert_spectrum_gap(S)
    e2, y2, rank2 = excited.solve(0.5 * (G + G.conj().T), S)
    assert rank2 == len(twice) - 1 == rank
    assert np.abs(e2 - energies).max() < 1e-9


def test_solve_refuses_shapes_and_a_zero_overlap():
    with pytest.raises(ValueError):
        excited.solve(np.eye(2), np.eye(3))
    with pytest.raises(ValueError):
        excited.solve(np.zeros((2, 2)), np.zeros((2, 2)))


# ---- the excitation operators -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_spatial,n_occ", [(2, 1), (3, 1), (4, 2)])
def test_excitation_operator_counts_and_action_on_the_reference(n_spatial, n_occ):
    singles, doubles = fermion.uccsd_excitations(n_spatial, n_occ)
    ne = len(singles) + len(doubles)
    n = 2 * n_spatial
    assert len(excited.excitation_operators(n_spatial, n_occ)) == ne + 1
    assert len(excited.excitation_operators(n_spatial, n_occ, identity=False)) == ne
    assert len(excited.excitation_operators(n_spatial, n_occ, deexcitations=True)) == 2 * ne + 1
    ops = excited.excitation_operators(n_spatial, n_occ, deexcitations=True, identity=False)
    hf = fermion.hf_integer(n, 2 * n_occ)
    ref = dense.basis_state(n, hf)
    bit = lambda q: 1 << (n - 1 - q)
    targets = [hf ^ bit(i) ^ bit(a) for i, a in singles] + [hf ^ bit(i) ^ bit(j) ^ bit(a) ^ bit(b) for i, j, a, b in doubles]
    for op, target in zip(ops[:ne], targets):
        out = dense.operator_matrix(op, sparse=True) @ ref
        assert abs(abs(out[target]) - 1.0) < 1e-14 and np.abs(np.delete(out, target)).max() < 1e-14
    for op, up in zip(ops[ne:], ops[:ne]):    # the de-excitations are the adjoints, and annihilate the reference
        assert np.abs(dense.operator_matrix(op, sparse=False) - dense.operator_matrix(up, sparse=False).conj().T).max() < 1e-14
        assert np.abs(dense.operator_matrix(op, sparse=True) @ ref).max() < 1e-14


def test_merged_pauli_sum_is_the_linear_combination():
    n = 4
    rng = np.random.default_rng(5)
    ops = sc.random_pool(rng, n, 5)
    y = rng.normal(size=5) + 1j * rng.normal(size=5)
    xs, zs, cs = excited.merged_pauli_sum(n, ops, y)
    psi = util.random_state(rng, n)
    from oracle import masks
    got = masks.apply_pauli_sum(psi, xs, zs, cs)
    want = sum(yj * (dense.operator_matrix(op, sparse=True) @ psi) for yj, op in zip(y, ops))
    assert np.abs(got - want).max() < 1e-13 and len(set(zip(xs.tolist(), zs.tolist()))) == len(xs)


# ---- the host planner under sanitizers ----------------------------------------------------------------------------------------------------
SAN_ENV = dict(ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


@pytest.fixture(scope="module")
def plan_check_exe(tmp_path_factory):
    src = os.path.join(ROOT, "tests", "cpu", "subspace_plan_check.cpp")
    exe = str(tmp_path_factory.mktemp("subspace_plan") / "subspace_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-o", exe, src])
    return exe


def test_subspace_plan_under_asan_ubsan(plan_check_exe):
    env = dict(os.environ, **SAN_ENV)
    for seed in ("7", "2025"):
        r = subprocess.run([plan_check_exe, seed], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "subspace plan ok" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]


# ---- the boundary cases of tests/test_gpu_subspace_edges.py -------------------------------------------------------------------------------
def _boundary_tuples():
    """(rows, m, with_h) of every named case, with and without h_out, and the same pools without rows"""
    out = []
    for (_, rows, m, _), _ in sc.EDGE_CASES.values():
        for t in ((rows, m, True), (rows, m, False), (0, m, True), (0, m, False)):
            if t not in out:
                out.append(t)
    # the unnamed cases: registers below one bitmap word (1 .. 2^n rows on 3 .. 5 qubits, m = 1 and 5), the dead and lone groups
    # (8 and 64 rows with m = 5, 3 rows with m = 4), the pool of three empty operators
    small = [(rows, m, True) for rows in (1, 2, 3, 4, 7, 8, 15, 16, 31, 32, 64) for m in (1, 5)] + [(3, 4, True), (0, 3, True)]
    return out + [t for t in small if t not in out]


def test_restated_plan_equals_the_host_planner_at_every_boundary_tuple(plan_check_exe):
    """``subspace_cases.plan`` against the lines subspace_plan_check prints in its boundary mode (under ASan + UBSan, a stand-alone
    program), which also places every row in its (slice, tile), every column block in its (column group, b), walks the pair lists at
    nb = 4, 5, 6 and the bitmap words of 1 .. 5 qubits"""
    tuples = _boundary_tuples()
    assert (0, 3, True) in tuples and (65536, 3, True) in tuples and (4101, 3, True) in tuples
    args = [f"{rows},{m},{int(with_h)},{sc.MI355X_CUS}" for rows, m, with_h in tuples]
    r = subprocess.run([plan_check_exe, "boundary"] + args, env=dict(os.environ, **SAN_ENV), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "subspace boundary ok" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("plan ")]
    assert len(lines) == len(tuples)
    for (rows, m, with_h), ln in zip(tuples, lines):
        printed = {k: int(v) for k, v in (kv.split("=") for kv in ln.split()[1:])}
        assert printed.pop("cus") == sc.MI355X_CUS
        want = sc.plan(rows, m, with_h, sc.MI355X_CUS)
        assert printed == {k: want[k] for k in sc.PLAN_FIELDS}, (ln, want)
    r = subprocess.run([plan_check_exe, "boundary", "12,0,1,256"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "bad tuple" in r.stdout


@pytest.mark.parametrize("name", sorted(sc.EDGE_CASES))
def test_each_named_case_lands_in_its_branch(name):
    """at the 256 CUs of an MI355X: the NB instantiated and its column groups, slices of more than one tile, the cap of 256 slices, the
    short last slice, grids smaller than the work"""
    p, branch = sc.edge_plan(name)
    assert branch(p), p
    (n, rows, m, with_h), _ = sc.EDGE_CASES[name]
    assert rows <= (1 << n) and p["rows"] * p["wpad"] * 16 <= 128 << 20


def test_the_branches_the_cases_are_named_for():
    plans = {name: sc.edge_plan(name)[0] for name in sc.EDGE_CASES}
    for m in sc.WIDTHS:
        p = plans[f"width dense m={m}"]
        assert p["sigma_blocks"] == (4 if m >= 193 else 2) and p["col_groups"] == (2 if m >= 257 or m == 192 else 1)
        live_in_last_group = p["nb"] - (p["col_groups"] - 1) * p["sigma_blocks"]
        assert live_in_last_group == {192: 1, 193: 4, 255: 4, 256: 4, 257: 1, 320: 1, 321: 2}[m]
    assert plans["width dense m=256"]["mb"] == 256 and plans["width dense m=257"]["mb"] - 257 == 63
    assert plans["gram two tiles"]["slice_rows"] > 16 and plans["gram slice cap"]["slices"] == 256
    p = plans["gram short last slice"]
    assert (p["slices"], p["slice_rows"], p["rows"] - (p["slices"] - 1) * p["slice_rows"]) == (129, 32, 5)
    p = plans["gram rows % 16 == 1"]
    assert p["rows"] - (p["slices"] - 1) * p["slice_rows"] == 17
    for name in ("stride dense", "stride sparse"):
        p = plans[name]
        assert p["sigma_grid"] == 8192 and p["sigma_grid"] * 4 < p["rows"] and p["expand_grid"] == 4096 and p["expand_grid"] * 256 < p["rows"] * p["mb"]
    # every earlier dense case of tests/test_gpu_subspace.py has one tile per slice and unstrided grids: the gap this table closes
    for n, m in [(2, 1), (5, 3), (6, 63), (7, 64), (7, 65), (10, 129)]:
        p = sc.plan(1 << n, m, True, sc.MI355X_CUS)
        assert p["slice_rows"] == 16 and p["sigma_blocks"] <= 2 and p["sigma_grid"] == p["row_tiles"]


# ---- the builders of the boundary cases ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,rows,xs", [(8, 42, [0, 0b10010110]), (13, 4101, [0]), (10, 592, [0, 0b1100000011, 0b0011000000, 0b101, 0b10]),
                                       (16, 40000, [0, 0x8001, 0x0180, 0x4002]), (10, 30, [0, 0b1000000001])])
def test_closed_support_state_has_the_rows_asked_for(n, rows, xs):
    rng = np.random.default_rng(rows)
    psi = sc.closed_support_state(rng, n, rows, xs)
    support = np.flatnonzero(psi)
    assert support.shape[0] == rows and abs(np.linalg.norm(psi) - 1.0) < 1e-14 and np.all(psi[support].imag != 0)
    for x in xs:
        assert np.array_equal(np.sort(support ^ x), support)
    ops = sc.pool_with_x(rng, n, 3, xs)
    assert sc.expected_rows(psi, n, ops) == rows
    assert len({w >> 6 for w in support.tolist()}) > 1                     # (the rows lie in several bitmap words)
    with pytest.raises(AssertionError):
        sc.closed_support_state(rng, n, rows + 1, [1, 2])


@pytest.mark.parametrize("n,m,xs", [(8, 321, [0, 0b10010110]), (5, 5, [1, 31, 4]), (3, 5, [1, 7, 2]), (6, 5, [0, 0b110000, 0b001111, 0b111100]),
                                    (9, 4, [0]), (4, 1, [0])])
def test_pool_with_x_uses_exactly_the_masks_given(n, m, xs):
    ops = sc.pool_with_x(np.random.default_rng(m), n, m, xs)
    packed = sc.packed_ops(n, ops)
    assert len(ops) == m and packed[0] == ([0], [0], [1.0 + 0j])
    assert {x for pxs, _, _ in packed for x in pxs} == set(xs) | {0}
    for pxs, pzs, pcs in packed[1:]:
        assert 1 <= len(pxs) and len(set(zip(pxs, pzs))) == len(pxs) and all(c.imag != 0 for c in pcs)
    if m > 1:                                                   # a pool of two operators still uses seven masks: seven strings in one
        assert {x for pxs, _, _ in sc.packed_ops(n, sc.pool_with_x(np.random.default_rng(m), n, 2, list(range(1, 8)))) for x in pxs} == set(range(8))


@pytest.mark.parametrize("ulp", [False, True])
def test_cancelling_hamiltonian_has_dead_groups_where_the_bits_agree(ulp):
    n = 6
    ham = sc.cancelling_hamiltonian(n, 0.25, ulp=ulp)
    xs = sc.handle_group_order(n, ham)
    assert xs == [0b000011, 0b001100, 0b110000] and ham.constant_coeff == 0.25 and len(ham.terms) == 6
    agree = sc.agreeing_indices(n)
    assert agree.tolist() == [i for i in range(64) if (i & 3) in (0, 3) and ((i >> 2) & 3) in (0, 3) and ((i >> 4) & 3) in (0, 3)]
    tiny = 64.0 * np.finfo(float).eps * sum(abs(t.coeff) for t in ham.terms[:2])      # the handle's threshold of one group
    for x in xs:
        for k in range(1 << n):
            d = sc.group_coefficient(n, ham, x, k)
            pair_agrees = bin(k & x).count("1") != 1
            if pair_agrees:
                assert d.imag == 0 and (abs(d.real) == np.finfo(float).eps / 2 if ulp else d == 0) and abs(d) <= tiny
            else:
                assert abs(d - 1.0) <= np.finfo(float).eps
    # the agreeing set is closed under the masks the GPU test moves it by, so no row there has a live group
    for x in [0b110000, 0b001111, 0b111100] + xs:
        assert np.array_equal(np.sort(agree ^ x), agree)
    # and the Hamiltonian is what it says: matrix elements only between rows whose pair bits differ
    mat = ham.get_matrix()
    assert np.abs(mat[np.ix_(agree, agree)] - 0.25 * np.eye(8)).max() <= np.finfo(float).eps


@pytest.mark.parametrize("ngroups,which", [(65, 0), (65, 63), (65, 64), (128, 0), (128, 63), (128, 64), (128, 127)])
def test_one_live_group_is_live_alone(ngroups, which):
    n = 9
    ham, psi, (a, b, c) = sc.one_live_group(n, ngroups, which)
    assert sc.handle_group_order(n, ham) == list(range(1, ngroups + 1)) and len(ham.terms) == ngroups
    assert np.flatnonzero(psi).tolist() == sorted((a, b, c)) and abs(np.linalg.norm(psi) - 1.0) < 1e-14
    ops = sc.pool_with_x(np.random.default_rng(which), n, 4, [0])
    assert sc.expected_rows(psi, n, ops) == 3
    R = (a, b, c)
    assert sc.live_groups(n, ham, R, a) == [which] and sc.live_groups(n, ham, R, b) == [which] and sc.live_groups(n, ham, R, c) == []
    assert (which % 64, which // 64) in ((0, 0), (63, 0), (0, 1), (63, 1))             # lane and batch of the sigma kernel
    # dropping the live group would move G_00 far beyond the tolerance
    coupling = abs(sc.group_coefficient(n, ham, which + 1, b) * np.conj(psi[a]) * psi[b])
    assert coupling > 1e4 * sc.g_bound(n, ops, ham)[0, 0]


def test_subspace_info_has_twenty_entries_declared():
    header = open(os.path.join(ROOT, "include", "ovqe_sv.h")).read()
    for k in range(14, 20):
        assert f"[{k}]" in header[header.index("of the last ovqe_subspace_matrices call"):header.index("int ovqe_subspace_info(")]
    text = open(os.path.join(ROOT, "openvqe_amd", "csrc", "sv_subspace_host.hpp")).read()
    for name, value in (("SIGMA_ROW_TILE", sc.SIGMA_ROW_TILE), ("SIGMA_MAX_BLOCKS", sc.SIGMA_MAX_BLOCKS)):
        assert f"constexpr int {name} = {value};" in text
    rdm_text = open(os.path.join(ROOT, "openvqe_amd", "csrc", "sv_rdm_host.hpp")).read()
    assert f"constexpr int GRAM_BLOCK = {sc.GRAM_BLOCK};" in rdm_text and f"constexpr int GRAM_MAX_SLICES = {sc.GRAM_MAX_SLICES};" in rdm_text
    assert f"constexpr int GRAM_TILE_BYTES = {sc.GRAM_TILE_ROWS * sc.GRAM_BLOCK * 16};" in rdm_text
