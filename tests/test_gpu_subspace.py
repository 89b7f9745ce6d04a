"""GPU tests of the subspace-expansion matrices (ovqe_subspace_matrices: csrc/sv_subspace_host.hpp, csrc/sv_subspace.hpp,
subspace_host.inc; Statevector.subspace_matrices / subspace_info; openvqe_amd/excited.py) against the checker of
tests/subspace_cases.py, with its tolerance: |dS_ij| <= 1e-12 a_i a_j, |dG_ij| <= 1e-10 (||H||_1 + |constant|) a_i a_j on real and
imaginary parts, a_j = sum_t |c_t| of operator j.  G is compared RAW (Phi^H Sigma as the device computed it)."""
import os
import re

import numpy as np
import pytest

from openvqe_amd import excited, fermion
from openvqe_amd.operators import Hamiltonian
from tests import subspace_cases as sc
from tests import util

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMA_GROUP_BATCH = 64    # sub::SIGMA_GROUP_BATCH: x-groups of H per hand-round of the sigma kernel
SIGMA_ROW_TILE = 4        # sub::SIGMA_ROW_TILE: rows per workgroup of the sigma kernel
INVALID, ALLOC, STATE = -1, -4, -5


@pytest.fixture(scope="module")
def SV(gpu_lib):
    from openvqe_amd.backend import Statevector
    return Statevector


def _pairs(m, with_h=True):
    nb = -(-m // 64)
    return nb * (nb + 1) // 2 + (nb * nb if with_h else 0)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def test_the_constants_restated_here_are_the_kernels():
    text = open(os.path.join(ROOT, "openvqe_amd", "csrc", "sv_subspace_host.hpp")).read()
    assert int(re.search(r"constexpr int SIGMA_GROUP_BATCH = (\d+);", text).group(1)) == SIGMA_GROUP_BATCH
    assert int(re.search(r"constexpr int SIGMA_ROW_TILE = (\d+);", text).group(1)) == SIGMA_ROW_TILE


# ---- 1. dense complex states ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(2, 1), (5, 3), (6, 63), (7, 64), (7, 65), (10, 129)])
def test_dense_complex_states(SV, n, m):
    rng = np.random.default_rng(1000 * n + m)
    ham = util.random_hamiltonian(rng, n, min(3 * n, 4 ** n - 1), constant=0.375)
    ops = sc.random_pool(rng, n, m)
    with SV(n) as sv:
        sv.set_hamiltonian(ham)
        sv.randomize(77 + n)
        psi = sv.get_state()
        G, S = sv.subspace_matrices(ops, raw=True)
        info = sv.subspace_info()
        after = sv.get_state()
        G2, S2 = sv.subspace_matrices(ops, raw=True)
        H, _ = sv.subspace_matrices(ops)
    assert abs(np.linalg.norm(psi) - 1.0) < 1e-12
    want_S, want_G, rows = sc.matrices(psi, n, ops, ham)
    sc.compare(f"dense n={n} m={m}", S, G, want_S, want_G, n, ops, ham)
    assert S.shape == (m, m) and G.shape == (m, m) and S.dtype == np.complex128
    assert np.array_equal(S, S.conj().T) and np.all(S.imag[np.diag_indices(m)] == 0.0)      # (values: -0.0 equals 0.0)
    assert rows == 1 << n and info["rows"] == rows and info["dense"] == 1 and info["m"] == m
    assert info["block_pairs"] == _pairs(m) and info["gram_launches"] == 1 and info["sigma_launches"] == 1 and info["expand_launches"] == 1
    assert info["store_bytes"] == rows * 2 * 64 * -(-m // 64) * 16
    assert np.array_equal(_bits(psi), _bits(after))
    assert np.array_equal(_bits(G), _bits(G2)) and np.array_equal(_bits(S), _bits(S2))
    assert np.array_equal(H, 0.5 * (G + G.conj().T))


# ---- 2. sparse real states ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_spatial,n_occ,seed", [(4, 2, 7), (6, 3, 11)])
def test_sparse_real_uccsd_states(SV, n_spatial, n_occ, seed):
    ham, gens, hf = fermion.synthetic_molecule(n_spatial, n_occ, seed)
    n = 2 * n_spatial
    ops = excited.excitation_operators(n_spatial, n_occ)
    theta = np.random.default_rng(seed).uniform(-0.2, 0.2, len(gens))
    with SV(n) as sv:
        sv.set_hamiltonian(ham)
        sv.set_ucc_program(gens, hf)
        e_before = sv.energy(theta)
        sv.prepare_state(theta)
        psi = sv.get_state()
        G, S = sv.subspace_matrices(ops, raw=True)
        info = sv.subspace_info()
        after = sv.get_state()
        e_after = sv.energy(theta)
    if n == 12:
        assert len(ops) == 118
    want_S, want_G, rows = sc.matrices(psi, n, ops, ham)
    sc.compare(f"uccsd n={n} m={len(ops)}", S, G, want_S, want_G, n, ops, ham)
    assert info["rows"] == rows and rows < (1 << n) and info["dense"] == 0, info
    assert info["block_pairs"] == _pairs(len(ops)) and info["store_bytes"] == rows * 2 * 64 * -(-len(ops) // 64) * 16
    assert np.array_equal(_bits(psi), _bits(after))
    assert np.float64(e_before).view(np.int64) == np.float64(e_after).view(np.int64)
    print(f"E = {e_before:.15f}, G00 / S00 = {(G[0, 0] / S[0, 0]).real:.15f}")
    assert abs(G[0, 0] / S[0, 0] - e_before) <= 1e-10 * sc.h_norm1(ham)


# ---- 3. shapes of the sigma kernel --------------------------------------------------------------------------------------------------------
def _sigma_case(SV, n, ham, psi, ops):
    with SV(n) as sv:
        sv.set_hamiltonian(ham)
        sv.set_state(psi)
        G, S = sv.subspace_matrices(ops, raw=True)
        info = sv.subspace_info()
    want_S, want_G, rows = sc.matrices(psi, n, ops, ham)
    sc.compare(f"sigma shape: {info['h_groups']} groups, {rows} rows", S, G, want_S, want_G, n, ops, ham)
    assert info["rows"] == rows
    return info


@pytest.mark.parametrize("ngroups,heavy", [(1, 5), (SIGMA_GROUP_BATCH - 1, 1), (SIGMA_GROUP_BATCH, 1), (SIGMA_GROUP_BATCH + 1, 1),
                                           (3, 45), (2 * SIGMA_GROUP_BATCH + 3, 2)])
def test_sigma_kernel_group_counts(SV, ngroups, heavy):
    """a diagonal-only Hamiltonian (one x-group, x = 0), B - 1 / B / B + 1 x-groups around the hand-round size B, one group of 45
    terms, more than two batches; dense complex state on 8 qubits"""
    n = 8
    rng = np.random.default_rng(31 * ngroups + heavy)
    ham = sc.hamiltonian_with_groups(rng, n, ngroups, heavy)
    info = _sigma_case(SV, n, ham, util.random_state(rng, n), sc.random_pool(rng, n, 5))
    assert info["h_groups"] == ngroups and info["dense"] == 1


def test_sigma_kernel_row_count_off_the_row_tile(SV):
    """a sparse complex state whose row set is no multiple of the sigma kernel's row tile (and lies in several bitmap words)"""
    n = 8
    rng = np.random.default_rng(9)
    psi = np.zeros(1 << n, np.complex128)
    where = [1, 66, 67, 130, 255]
    psi[where] = rng.normal(size=5) + 1j * rng.normal(size=5)
    psi /= np.linalg.norm(psi)
    ops = sc.random_pool(rng, n, 4)
    ham = sc.hamiltonian_with_groups(rng, n, 70, 3)
    info = _sigma_case(SV, n, ham, psi, ops)
    assert info["dense"] == 0 and info["rows"] % SIGMA_ROW_TILE != 0 and info["rows"] < (1 << n), info


# ---- 4. h_out NULL ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(6, 5), (7, 65)])
def test_overlap_alone_needs_no_hamiltonian(SV, n, m):
    rng = np.random.default_rng(n + m)
    ops = sc.random_pool(rng, n, m)
    ham = util.random_hamiltonian(rng, n, 10, constant=-0.5)
    with SV(n) as sv:
        sv.randomize(3)
        S_alone = sv.subspace_matrices(ops, hamiltonian=False)       # no Hamiltonian on the handle
        info = sv.subspace_info()
        sv.set_hamiltonian(ham)
        _, S_full = sv.subspace_matrices(ops)
        psi = sv.get_state()
    assert np.array_equal(_bits(S_alone), _bits(S_full))
    assert info["block_pairs"] == _pairs(m, with_h=False) and info["sigma_launches"] == 0 and info["h_groups"] == 0
    assert info["store_bytes"] == (1 << n) * 64 * -(-m // 64) * 16
    want_S, _, _ = sc.matrices(psi, n, ops, None)
    sc.compare(f"S alone n={n} m={m}", S_alone, None, want_S, None, n, ops, None)


# ---- 5. an operator with no terms -------------------------------------------------------------------------------------------------------
def test_operator_without_terms_gives_a_zero_row_and_column(SV):
    n, m = 6, 6
    rng = np.random.default_rng(12)
    ops = sc.random_pool(rng, n, m)
    ham = util.random_hamiltonian(rng, n, 10, constant=0.25)
    holed = ops[:3] + [Hamiltonian(n, [], 0.0)] + ops[3:]
    keep = [0, 1, 2, 4, 5, 6]
    with SV(n) as sv:
        sv.set_hamiltonian(ham)
        sv.randomize(21)
        G, S = sv.subspace_matrices(ops, raw=True)
        Gh, Sh = sv.subspace_matrices(holed, raw=True)
    for M in (Gh, Sh):
        assert np.all(M[3] == 0) and np.all(M[:, 3] == 0)
    assert np.array_equal(_bits(Sh[np.ix_(keep, keep)]), _bits(S)) and np.array_equal(_bits(Gh[np.ix_(keep, keep)]), _bits(G))


# ---- 6. the cap of the store ------------------------------------------------------------------------------------------------------------
def test_store_beyond_its_cap_is_refused_and_the_handle_stays_usable(SV):
    from openvqe_amd._lib import BackendError
    n, m = 10, 129
    rng = np.random.default_rng(6)
    ops = sc.random_pool(rng, n, m)
    ham = util.random_hamiltonian(rng, n, 20, constant=0.5)
    need = (1 << n) * 2 * 192 * 16
    with SV(n) as sv:
        sv.set_hamiltonian(ham)
        sv.randomize(2)
        sv.set_option("subspace_workspace_mb", 1)
        with pytest.raises(BackendError, match=str(need)):
            sv.subspace_matrices(ops)
        sv.set_option("subspace_workspace_mb", 64)
        G, S = sv.subspace_matrices(ops, raw=True)
        info = sv.subspace_info()
        psi = sv.get_state()
    assert info["store_bytes"] == need
    want_S, want_G, _ = sc.matrices(psi, n, ops, ham)
    sc.compare("after the refusal", S, G, want_S, want_G, n, ops, ham)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------
def _raw(sv, n_ops, offsets, xs, zs, cre, with_h=True):
    m = max(n_ops, 1)
    h_out, s_out = np.zeros(2 * m * m), np.zeros(2 * m * m)
    rc = sv._L.ovqe_subspace_matrices(sv._h, n_ops, np.asarray(offsets, np.int64), np.asarray(xs, np.uint64), np.asarray(zs, np.uint64),
                                      np.asarray(cre, np.float64), None, h_out if with_h else None, s_out)
    return rc, (sv._L.ovqe_last_error(sv._h) or b"").decode(), s_out


def test_refusals_leave_the_handle_usable(SV):
    n = 4
    ham = util.random_hamiltonian(np.random.default_rng(1), n, 6, constant=0.1)
    good = ([0, 1, 2], [0, 3], [0, 1], [1.0, 0.5])
    with SV(n) as sv:
        sv.randomize(1)
        rc, msg, _ = _raw(sv, 2, *good)                               # h_out asked for, no Hamiltonian
        assert rc == STATE and "Hamiltonian" in msg
        rc, _, s = _raw(sv, 2, *good, with_h=False)
        assert rc == 0 and abs(s[0] - 1.0) < 1e-12
        sv.set_hamiltonian(ham)
        assert _raw(sv, 2, *good)[0] == 0
        rc, msg, _ = _raw(sv, 0, [0], [0], [0], [1.0])
        assert rc == INVALID and "n_ops" in msg
        rc, msg, _ = _raw(sv, 2, [0, 1, 2], [0, 1 << n], [0, 1], [1.0, 0.5])
        assert rc == INVALID and "beyond the register" in msg
        rc, msg, _ = _raw(sv, 2, [0, 1, 2], [0, 3], [1 << n, 1], [1.0, 0.5])
        assert rc == INVALID and "beyond the register" in msg
        rc, msg, _ = _raw(sv, 2, [0, 2, 1], [0, 3], [0, 1], [1.0, 0.5])
        assert rc == INVALID and "monotone" in msg
        sv.set_option("real_state", 1)
        rc, msg, _ = _raw(sv, 2, *good)
        assert rc == STATE and "real_state" in msg
        sv.set_option("real_state", 0)
        assert _raw(sv, 2, *good)[0] == 0
        assert sv.subspace_info()["m"] == 2
    with SV(n, n_global=1, shard_index=0) as sv:
        rc, msg, _ = _raw(sv, 2, *good, with_h=False)
        assert rc == STATE and "shard" in msg
        assert sv.subspace_info()["m"] == 0                            # zeros before the first successful call


# ---- 8. end to end ------------------------------------------------------------------------------------------------------------------------
def test_excited_states_of_a_three_orbital_molecule(SV):
    """synthetic_molecule(3, 1, 5), excitations + de-excitations: the nine eigenvalues of the sector, then the second Ritz state in
    the buffer.  psi is the sector's ground state: ovqe_sector_ground_state answers OVQE_ERR_STATE on a 6-qubit register (its
    tables need a support list, which exists from 12 qubits on), so the block's lowest eigenvector from dense numpy is loaded
    instead; the 12-qubit test below takes psi from ovqe_sector_ground_state itself."""
    mol = sc.Molecule(3, 1, 5)
    ops = mol.pool(deexcitations=True)
    with SV(mol.n) as sv:
        sv.set_hamiltonian(mol.ham)
        sv.set_state(mol.psi)
        e0, res = sv.expectation(mol.ham), 0.0
        energies, y, rank = excited.qse(sv, ops)
        info = sv.subspace_info()
        norm2_before = excited.load_ritz_state(sv, ops, y[:, 1])
        e1 = sv.expectation(mol.ham)
        norm2 = sv.norm2()
    print(f"E0 = {e0:.12f} (residual {res:.2e}), QSE {energies}, exact {mol.block_energies}, rows {info['rows']}")
    assert rank == 9 and len(ops) == 17
    assert np.abs(energies - mol.block_energies).max() < 1e-9
    assert abs(e0 - mol.block_energies[0]) < 1e-9
    assert abs(e1 - energies[1]) <= 1e-10 * sc.h_norm1(mol.ham)
    assert abs(norm2 - 1.0) < 1e-12 and abs(norm2_before - 1.0) < 1e-8


def test_ritz_states_around_the_vector_left_by_sector_ground_state(SV):
    """synthetic_molecule(6, 3, 11), 12 qubits: ovqe_sector_ground_state leaves the sector's ground state psi in the buffer; with
    the identity in the pool the lowest Ritz value is <psi|H|psi> = E0 and no Ritz value lies below it.  The second Ritz state goes
    back into the buffer: its <H> is y^H G y, whose error is the entry tolerance of G weighted by |y_i| |y_j|:
    1e-10 ||H||_1 (sum_i |y_i| a_i)^2."""
    ham, _, hf = fermion.synthetic_molecule(6, 3, 11)
    ops = excited.excitation_operators(6, 3)
    with SV(12) as sv:
        sv.set_hamiltonian(ham)
        sv.init_basis(hf)
        e0, res, _ = sv.sector_ground_state(tol=1e-12)
        energies, y, rank = excited.qse(sv, ops)
        info = sv.subspace_info()
        excited.load_ritz_state(sv, ops, y[:, 1])
        e1, norm2 = sv.expectation(ham), sv.norm2()
    bound = 1e-10 * sc.h_norm1(ham) * float(np.abs(y[:, 1]) @ sc.weights(12, ops)) ** 2
    print(f"E0 = {e0:.12f} (residual {res:.2e}), Ritz {energies[:3]}, rank {rank}, rows {info['rows']}, <H>_1 = {e1:.12f}, bound {bound:.2e}")
    assert len(ops) == 118 and 2 <= rank <= 118 and info["dense"] == 0 and 400 <= info["rows"] < 4096
    assert abs(energies[0] - e0) < 1e-9 and np.all(np.diff(energies) >= 0)
    assert abs(e1 - energies[1]) <= max(bound, 1e-10 * sc.h_norm1(ham)) and abs(norm2 - 1.0) < 1e-12
