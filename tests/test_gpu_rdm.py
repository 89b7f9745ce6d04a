"""GPU tests of the one- and two-particle density matrices of the resident state (ovqe_rdm: csrc/sv_rdm.hpp, rdm_host.inc;
Statevector.rdm1 / rdm2 / rdm_info; openvqe_amd/rdm.py) against the two oracles of tests/rdm_cases.py."""
import ctypes

import numpy as np
import pytest

from openvqe_amd import fermion, rdm
from openvqe_amd.operators import Hamiltonian
from tests import rdm_cases

pytestmark = pytest.mark.gpu

TOL = 1e-12   # the project's amplitude bar


@pytest.fixture(scope="module")
def SV(gpu_lib):
    from openvqe_amd.backend import Statevector
    return Statevector


# ---- dense random complex states ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 5, 6, 7, 9, 12, 13])
def test_dense_complex_state_against_the_pauli_oracle(SV, n):
    """n = 2: P = 1; 3 / 5: odd widths, a bitmap below one word; 6: exactly one word; 7 and up: several words; 9: P = 36 < 64;
    12 / 13: P = 66 / 78 — two column blocks, the off-diagonal block pair and its mirror, a last block of 2 / 14 valid columns.
    Real AND imaginary parts are compared: which side is conjugated is part of the contract."""
    upper = n >= 12
    with SV(n) as sv:
        sv.randomize(20250227 + n)
        psi = sv.get_state()
        g1 = sv.rdm1()
        i1 = sv.rdm_info()
        d2 = sv.rdm2(packed=True)
        i2 = sv.rdm_info()
        psi_after = sv.get_state()
    assert np.array_equal(psi, psi_after)                       # the state is only read
    for order, got, info in ((1, g1, i1), (2, d2, i2)):
        want = rdm_cases.pauli_rdm(psi, n, order, upper_only=upper)
        W = n if order == 1 else n * (n - 1) // 2
        assert got.shape == (W, W)
        mask = np.triu(np.ones((W, W), bool)) if upper else np.ones((W, W), bool)
        err = np.abs(got[mask] - want[mask]).max()
        print(f"n={n} order={order} max|diff|={err:.3e} info={info}")
        assert err <= TOL
        assert np.array_equal(got, got.conj().T)                # Hermitian to the bit
        assert info["real"] == 0 and info["nonzeros"] == 1 << n
        assert info["rows"] == (1 << n) - sum(1 for k in range(1 << n) if n - bin(k).count("1") < order)
        assert info["block_pairs"] == ((W + 63) // 64) * ((W + 63) // 64 + 1) // 2


# ---- sparse real states: UCCSD at non-zero angles ----------------------------------------------------------------------------------
class Sparse:
    def __init__(self, SV, n, ham, gens, hf, hpq, hpqrs, constant, n_elec, seed, workspace_mb=None):
        """constant: the one the integrals come with (ham.constant_coeff also holds the identity strings of the Jordan-Wigner image)"""
        self.n, self.ham, self.hpq, self.hpqrs, self.constant, self.n_elec = n, ham, hpq, hpqrs, float(constant), n_elec
        rng = np.random.default_rng(seed)
        self.theta = rng.uniform(-0.2, 0.2, len(gens))
        with SV(n) as sv:
            if workspace_mb is not None:
                sv.set_option("rdm_workspace_mb", workspace_mb)
            sv.set_hamiltonian(ham)
            sv.set_ucc_program(gens, hf)
            self.e = sv.energy(self.theta)                      # the Hamiltonian kernels' energy
            sv.prepare_state(self.theta)
            self.psi = sv.get_state()
            self.g1 = sv.rdm1()
            self.i1 = sv.rdm_info()
            self.d2 = sv.rdm2(packed=True)
            self.i2 = sv.rdm_info()
            self.g1_again, self.d2_again = sv.rdm1(), sv.rdm2(packed=True)
        self.idx = np.flatnonzero(self.psi)
        self.l1 = float(sum(abs(t.coeff) for t in ham.terms)) + abs(ham.constant_coeff)


def _pad(hpq, hpqrs, n):
    m = hpq.shape[0]
    a, b = np.zeros((n, n)), np.zeros((n, n, n, n))
    a[:m, :m] = hpq
    b[:m, :m, :m, :m] = hpqrs
    return a, b


@pytest.fixture(scope="module")
def synth12(SV):
    h, g = fermion.synthetic_integrals(6, 41)
    hpq, hpqrs = fermion.spin_orbital_integrals(h, g)
    ham, gens, hf = fermion.synthetic_molecule(6, 3, 41)
    return Sparse(SV, 12, ham, gens, hf, hpq, hpqrs, 0.0, 6, 1)


def _h2o():
    from openvqe_amd import chem
    mol = chem.molecule("H2O")
    mol.rhf()
    hpq, hpqrs = fermion.spin_orbital_integrals(mol.h_mo, mol.eri_mo)      # what mol.jw_hamiltonian() is built from
    return mol, (hpq, hpqrs), mol.jw_hamiltonian(), fermion.uccsd_generators(mol.nao, mol.n_elec // 2), mol.hf_init()


@pytest.fixture(scope="module")
def h2o_parts():
    return _h2o()


@pytest.fixture(scope="module")
def h2o(SV, h2o_parts):
    mol, (hpq, hpqrs), ham, gens, hf = h2o_parts
    return Sparse(SV, 14, ham, gens, hf, hpq, hpqrs, mol.nuclear_repulsion(), mol.n_elec, 2)


@pytest.fixture(scope="module")
def synth17(SV):
    """a 16-spin-orbital synthetic molecule on a 17-qubit register (the last orbital stays empty): odd n, P = 136, three column blocks"""
    h, g = fermion.synthetic_integrals(8, 43)
    hpq, hpqrs = _pad(*fermion.spin_orbital_integrals(h, g), 17)
    ham16, gens, hf16 = fermion.synthetic_molecule(8, 2, 43)
    ham = Hamiltonian(17, ham16.terms, ham16.constant_coeff, do_clean_up=False)
    return Sparse(SV, 17, ham, gens, hf16 << 1, hpq, hpqrs, 0.0, 4, 3)


@pytest.mark.parametrize("case", ["synth12", "h2o", "synth17"])
def test_sparse_real_state(case, request):
    """oracle (b), the real form, the row count from the state itself, traces, exact hermiticity, the energy re-assembled from the
    integrals against the HAMILTONIAN kernels' energy, determinism"""
    c = request.getfixturevalue(case)
    n, N = c.n, c.n_elec
    assert abs(np.linalg.norm(c.psi) - 1.0) < 1e-12 and np.abs(c.psi.imag).max() == 0.0 and 1 < len(c.idx) <= (1 << n) // 4
    for order, got, info in ((1, c.g1, c.i1), (2, c.d2, c.i2)):
        want = rdm_cases.det_rdm(c.idx, c.psi[c.idx], n, order)
        err = np.abs(got - want).max()
        print(f"{case} order={order} max|diff|={err:.3e} info={info}")
        assert err <= TOL
        assert info["real"] == 1 and info["nonzeros"] == len(c.idx)
        assert info["rows"] == rdm_cases.expected_rows(c.idx, n, order)
        assert np.array_equal(got, got.conj().T) and np.abs(got.imag).max() == 0.0
    assert c.i2["block_pairs"] == {12: 3, 14: 3, 17: 6}[n]
    assert abs(np.trace(c.g1).real - N) < 1e-12
    assert abs(np.trace(c.d2).real - N * (N - 1) / 2) < 1e-12
    g2 = rdm.unpack_rdm2(c.d2, n)
    e_rdm = rdm.energy(c.hpq, c.hpqrs, c.constant, c.g1, g2)
    print(f"{case} E(rdm)={e_rdm:.15f} E(H)={c.e:.15f} |H|_1={c.l1:.3f}")
    assert abs(e_rdm - c.e) <= 1e-10 * c.l1
    assert np.array_equal(c.g1, c.g1_again) and np.array_equal(c.d2, c.d2_again)     # bit-identical from call to call


def _singlet_angles(n_spatial, n_occ_spatial, rng):
    """non-zero UCCSD angles that keep a closed-shell determinant a singlet: the alpha and the beta single i -> a share their angle
    (all alpha generators commute with all beta generators, so the singles are one orbital rotation applied to both spins) and of
    the doubles only the pair excitations (i alpha, i beta) -> (a alpha, a beta) are switched on — each a singlet operator"""
    singles, doubles = fermion.uccsd_excitations(n_spatial, n_occ_spatial)
    t1 = rng.uniform(-0.2, 0.2, (n_spatial, n_spatial))
    theta = [t1[i // 2, a // 2] for i, a in singles]
    theta += [rng.uniform(-0.2, 0.2) if (i % 2 == 0 and j == i + 1 and a % 2 == 0 and b == a + 1) else 0.0 for i, j, a, b in doubles]
    return np.array(theta)


def test_closed_shell_h2o_is_a_singlet(SV, h2o, h2o_parts):
    """<S^2> = 0 on the closed-shell H2O state at spin-symmetric angles; at the generic angles of the fixture (independent angles per
    spin-orbital excitation: a spin-contaminated state) the value from the density matrices is the operator's expectation value"""
    mol, _, ham, gens, hf = h2o_parts
    theta = _singlet_angles(mol.nao, mol.n_elec // 2, np.random.default_rng(7))
    assert np.count_nonzero(theta) >= 30
    with SV(14) as sv:
        sv.set_ucc_program(gens, hf)
        sv.prepare_state(theta)
        psi = sv.get_state()
        g1, g2 = sv.rdm1(), sv.rdm2()
    assert abs(psi[hf]) < 0.999                                   # the angles moved the state
    N, sz, s2 = rdm.spin_expectations(g1, g2)
    print(f"H2O singlet angles: N={N:.15f} Sz={sz:.3e} S2={s2:.3e}")
    assert abs(N - 10) < 1e-12 and abs(sz) < 1e-12 and abs(s2) <= 1e-10
    noons, _ = rdm.natural_occupations(g1)
    assert abs(noons.sum() - 10) < 1e-12 and np.all(noons > -1e-12) and np.all(noons < 2 + 1e-12)
    N, sz, s2 = rdm.spin_expectations(h2o.g1, rdm.unpack_rdm2(h2o.d2, 14))
    want = rdm_cases.s2_expectation(h2o.psi, 14)
    print(f"H2O generic angles: N={N:.15f} Sz={sz:.3e} S2={s2:.12f} operator {want:.12f}")
    assert abs(N - 10) < 1e-12 and abs(sz) < 1e-12 and abs(s2 - want) <= 1e-10


def test_row_chunks_give_the_one_chunk_result(SV, h2o, h2o_parts):
    """"rdm_workspace_mb" = 1: 1024 rows of P = 91 -> 128 doubles per chunk"""
    mol, (hpq, hpqrs), ham, gens, hf = h2o_parts
    small = Sparse(SV, 14, ham, gens, hf, hpq, hpqrs, mol.nuclear_repulsion(), mol.n_elec, 2, workspace_mb=1)
    assert h2o.i2["chunks"] == 1 and small.i2["chunks"] >= 3 and small.i2["gram_launches"] == small.i2["chunks"]
    assert small.i2["workspace_bytes"] <= 1 << 20 and small.i2["rows"] == h2o.i2["rows"]
    assert np.array_equal(small.psi, h2o.psi)
    for a, b in ((small.g1, h2o.g1), (small.d2, h2o.d2)):
        err = np.abs(a - b).max()
        print(f"chunks={small.i2['chunks']} max|diff|={err:.3e}")
        assert err <= 1e-13


def test_workspace_minimum_is_one_tile(SV):
    with SV(9) as sv:
        sv.randomize(5)
        a = sv.rdm2(packed=True)
        sv.set_option("rdm_workspace_mb", 0)
        b = sv.rdm2(packed=True)
        info = sv.rdm_info()
    assert info["chunks"] == -(-info["rows"] // 16) and info["workspace_bytes"] == 16 * 64 * 16
    assert np.abs(a - b).max() <= 1e-13


def test_eigenvector_left_by_sector_ground_state(SV, synth12):
    """a state no program prepared: the FCI vector of the determinant's sector; its energy from the density matrices equals the
    eigenvalue within the solver's residual bound"""
    c = synth12
    with SV(12) as sv:
        sv.set_hamiltonian(c.ham)
        sv.init_basis(fermion.hf_integer(12, 6))
        e, res, _ = sv.sector_ground_state(tol=1e-12)
        g1, g2 = sv.rdm1(), sv.rdm2()
        info = sv.rdm_info()
    e_rdm = rdm.energy(c.hpq, c.hpqrs, c.constant, g1, g2)
    print(f"E(fci)={e:.15f} E(rdm)={e_rdm:.15f} residual={res:.3e}")
    assert info["real"] == 1 and info["nonzeros"] <= 400
    assert abs(e_rdm - e) <= 1e-9
    N, sz, s2 = rdm.spin_expectations(g1, g2)
    assert abs(N - 6) < 1e-12 and abs(sz) < 1e-12


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def _refused(sv, order, out):
    rc = sv._L.ovqe_rdm(sv._h, order, out)
    msg = sv._L.ovqe_last_error(sv._h)
    return rc, (msg or b"").decode()


def test_refusals(SV):
    from openvqe_amd import _lib
    INVALID, STATE = -1, -5
    out = np.zeros(2 * 16 * 16)
    with SV(4) as sv:
        sv.init_basis(3)
        for order in (0, 3, -1):
            rc, msg = _refused(sv, order, out)
            assert rc == INVALID and msg
        raw = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p)(("ovqe_rdm", sv._L))
        assert raw(sv._h, 1, None) == INVALID and sv._L.ovqe_last_error(sv._h)
        sv.set_option("real_state", 1)
        rc, msg = _refused(sv, 1, out)
        assert rc == STATE and "real_state" in msg
        sv.set_option("real_state", 0)
        assert sv.rdm1()[2, 2] == 1.0 and sv.rdm1()[3, 3] == 1.0 and np.trace(sv.rdm1()) == 2.0     # |0011>: orbitals 2 and 3
        with pytest.raises(_lib.BackendError):
            sv.set_option("rdm_workspace", 1)
    with SV(1) as sv:
        sv.init_basis(1)
        rc, msg = _refused(sv, 2, out)
        assert rc == INVALID and msg
        assert sv.rdm1()[0, 0] == 1.0
    with SV(4, n_global=1, shard_index=0) as sv:
        for order in (1, 2):
            rc, msg = _refused(sv, order, out)
            assert rc == STATE and msg
