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
def test_subspace_plan_under_asan_ubsan(tmp_path):
    src = os.path.join(ROOT, "tests", "cpu", "subspace_plan_check.cpp")
    exe = str(tmp_path / "subspace_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-o", exe, src])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    for seed in ("7", "2025"):
        r = subprocess.run([exe, seed], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "subspace plan ok" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
