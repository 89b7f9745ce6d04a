"""CPU tests of the density matrices (ovqe_rdm): the oracles of tests/rdm_cases.py against each other, the numpy helpers of
openvqe_amd/rdm.py against dense operators, the new symbols in header / cdef / ctypes table, and the host-side plan
(openvqe_amd/csrc/sv_rdm_host.hpp) replayed by tests/cpu/rdm_plan_check.cpp under ASan + UBSan with g++ alone."""
import os
import subprocess

import numpy as np
import pytest

from openvqe_amd import fermion, rdm
from oracle import masks
from tests import rdm_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_state(n, seed):
    rng = np.random.default_rng(seed)
    psi = rng.normal(size=1 << n) + 1j * rng.normal(size=1 << n)
    return psi / np.linalg.norm(psi)


@pytest.fixture(scope="module")
def six():
    """a random complex 6-qubit state (no particle-number or spin symmetry) with its density matrices from oracle (a)"""
    psi = _random_state(6, 11)
    g1 = rdm_cases.pauli_rdm(psi, 6, 1)
    d2 = rdm_cases.pauli_rdm(psi, 6, 2)
    return psi, g1, d2, rdm.unpack_rdm2(d2, 6)


@pytest.mark.parametrize("n", [4, 6])
def test_determinant_oracle_equals_pauli_oracle(n):
    psi = _random_state(n, 100 + n)
    idx = np.arange(1 << n)
    for order in (1, 2):
        a = rdm_cases.pauli_rdm(psi, n, order)
        b = rdm_cases.det_rdm(idx, psi, n, order)
        assert a.shape == b.shape
        assert np.abs(a - b).max() < 1e-14
        assert np.abs(a - a.conj().T).max() < 1e-14
        assert rdm_cases.expected_rows(idx, n, order) == (1 << n) - sum(1 for k in idx if n - bin(k).count("1") < order)


@pytest.mark.parametrize("n", [4, 6])
def test_vectorised_oracle_equals_both_oracles(n):
    """vec_rdm (the oracle of the large GPU cases) on a random complex state: every element against the Pauli sums and against the
    determinant loop, and its row count against the set of shadows"""
    psi = _random_state(n, 300 + n)
    idx = np.arange(1 << n)
    for order in (1, 2):
        got, rows = rdm_cases.vec_rdm(idx, psi, n, order)
        a = rdm_cases.pauli_rdm(psi, n, order)
        b = rdm_cases.det_rdm(idx, psi, n, order)
        assert got.shape == a.shape
        assert np.abs(got - a).max() < 1e-14 and np.abs(got - b).max() < 1e-14
        assert rows == rdm_cases.expected_rows(idx, n, order)
        small, rows_small = rdm_cases.vec_rdm(idx, psi, n, order, block_rows=5)      # several row blocks, a short last one
        assert rows_small == rows and np.abs(small - a).max() < 1e-14


@pytest.mark.parametrize("complex_amps", [False, True])
def test_vectorised_oracle_on_a_sparse_state(complex_amps):
    """n = 10, 60 determinants of no particular particle number: the signs of orbitals far apart, rows shared by few determinants"""
    n = 10
    idx, amps = rdm_cases.sparse_state(n, 60, 77, complex_amps)
    assert len(set(bin(int(i)).count("1") for i in idx)) > 3
    for order in (1, 2):
        got, rows = rdm_cases.vec_rdm(idx, amps, n, order)
        want = rdm_cases.det_rdm(idx, amps, n, order)
        assert np.abs(got - want).max() < 1e-14
        assert rows == rdm_cases.expected_rows(idx, n, order)
        assert (np.abs(got.imag).max() > 0) == complex_amps


def test_unpack_antisymmetry(six):
    _, _, d2, g2 = six
    n = 6
    assert g2.shape == (n,) * 4
    assert np.abs(g2 + g2.transpose(1, 0, 2, 3)).max() == 0.0
    assert np.abs(g2 + g2.transpose(0, 1, 3, 2)).max() == 0.0
    assert np.abs(g2 - g2.transpose(1, 0, 3, 2)).max() == 0.0
    for p in range(n):
        assert np.abs(g2[p, p]).max() == 0.0 and np.abs(g2[:, :, p, p]).max() == 0.0
    pr = rdm.pair_index(n)
    for i, (p, q) in enumerate(pr):
        for j, (r, s) in enumerate(pr):
            assert g2[p, q, r, s] == -d2[i, j]
    # an element off the packed triangle against its own operator: Gamma[q, p, r, s], q > p
    psi = six[0]
    assert abs(g2[3, 1, 0, 4] - rdm_cases.pauli_expectation(psi, n, [(3, True), (1, True), (0, False), (4, False)])) < 1e-14
    with pytest.raises(ValueError):
        rdm.unpack_rdm2(d2, 5)


def test_energy_identity_against_the_dense_hamiltonian(six):
    psi, g1, _, g2 = six
    h, g = fermion.synthetic_integrals(3, 5)
    hpq, hpqrs = fermion.spin_orbital_integrals(h, g)
    const = 0.375
    ham = fermion.jw_molecular_hamiltonian(hpq, hpqrs, const)
    from openvqe_amd.operators import pack_terms
    xs, zs, cs = pack_terms(6, ham.terms)
    want = masks.expectation(psi, [int(x) for x in xs], [int(z) for z in zs], list(cs), ham.constant_coeff)
    assert abs(rdm.energy(hpq, hpqrs, const, g1, g2) - want) < 1e-13
    from openvqe_amd.chem import Problem
    prob = Problem(h, g, const, 2, [2.0, 0.0, 0.0], [0.0, 0.0, 0.0])
    assert prob.rdm_energy(g1, g2) == rdm.energy(hpq, hpqrs, const, g1, g2)


def test_spin_expectations_against_the_operators(six):
    psi, g1, _, g2 = six
    n = 6
    N, sz, s2 = rdm.spin_expectations(g1, g2)
    num = rdm_cases.number_operator(n, [(p, 1.0) for p in range(n)])
    szd = rdm_cases.number_operator(n, [(p, 0.5 if p % 2 == 0 else -0.5) for p in range(n)])
    assert abs(N - np.vdot(psi, num * psi).real) < 1e-14
    assert abs(sz - np.vdot(psi, szd * psi).real) < 1e-14
    assert abs(s2 - rdm_cases.s2_expectation(psi, n)) < 1e-14


def test_natural_occupations_of_a_closed_shell_determinant():
    n = 6
    g1 = np.diag([1.0, 1.0, 1.0, 1.0, 0.0, 0.0]).astype(np.complex128)
    noons, orbs = rdm.natural_occupations(g1)
    assert np.allclose(noons, [2.0, 2.0, 0.0]) and orbs.shape == (3, 3)
    assert np.allclose(rdm.spin_summed_rdm1(g1), np.diag([2.0, 2.0, 0.0]))
    psi = _random_state(n, 3)
    g = rdm_cases.pauli_rdm(psi, n, 1)
    w, v = rdm.natural_occupations(g)
    d = rdm.spin_summed_rdm1(g)
    assert np.all(np.diff(w) <= 0) and np.abs(v @ np.diag(w) @ v.conj().T - d).max() < 1e-14


def test_rdm_symbols_are_declared_everywhere():
    from openvqe_amd import _lib
    header = open(os.path.join(ROOT, "include", "ovqe_sv.h")).read()
    cdef = open(os.path.join(ROOT, "include", "ovqe_sv.cdef.h")).read()
    for name in ("ovqe_rdm", "ovqe_rdm_info"):
        assert name + "(" in header and name + "(" in cdef and name in _lib.SIGNATURES
    assert '"rdm_workspace_mb"' in header and "Jordan-Wigner" in header.replace("JORDAN-WIGNER", "Jordan-Wigner")
    from openvqe_amd.backend import Statevector
    from openvqe_amd.partitioned import PartitionedStatevector
    for m in ("rdm1", "rdm2", "rdm_info"):
        assert callable(getattr(Statevector, m))
    for m in ("rdm1", "rdm2"):
        with pytest.raises(NotImplementedError):
            getattr(PartitionedStatevector, m)(None)


def test_rdm_plan_under_asan_ubsan(tmp_path):
    src = os.path.join(ROOT, "tests", "cpu", "rdm_plan_check.cpp")
    exe = str(tmp_path / "rdm_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-o", exe, src])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    for seed in ("7", "2025"):
        r = subprocess.run([exe, seed], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "rdm plan ok" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
