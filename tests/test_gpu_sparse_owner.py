"""The restricted Hamiltonian as owner pieces in the workgroup geometry of the rows form (k_sparse_vqe_rows_shared, sv_sparse.hpp;
packer: sparse_pack.hpp): the shipped instances against the per-wave geometry (k_sparse_vqe_rows<2>, testing option
"sparse_shared" = 0) on every energy of a batch — H2O and LiH, batches whose last work item holds 1 ... 7 evaluations and batches
of more work items than the persistent grid has workgroups — what ``program_info`` says about the pieces, and the selection's
fall-back when the entries do not pack (testing option "sparse_pack" = 0).

The bound is the one tests/test_gpu_sparse_shared.py uses between the two geometries: 1e-12 x max(1, ||H||_1) — both sum the same
products c a_i a_j of the same amplitudes (the circuits are the same instructions) in different orders."""
import numpy as np
import pytest

from tests.test_gpu_sparse import _thetas_with_nan_tail, h2o, testing_lib  # noqa: F401
from tests.test_gpu_sparse_shared import H2O_GEOMETRY, LIH_GEOMETRY, T, lih  # noqa: F401

pytestmark = pytest.mark.gpu

NT = 256
# sparse_host.inc: SHARED_37 / SHARED_13 — pieces per thread, slots per piece
H2O_SHAPE = (4, 10)
LIH_SHAPE = (1, 17)


def _both_geometries(case, B, seed, want):
    from openvqe_amd.backend import Statevector
    rng = np.random.default_rng(seed)
    full = _thetas_with_nan_tail(rng, B, case.K, extra=64)
    out = {}
    for shared in (1, 0):
        with Statevector(case.n) as sv:
            sv.set_option("sparse_shared", shared)
            sv.set_hamiltonian(case.H)
            case.program(sv)
            out[shared] = sv.energy_batch(full[:B])
            assert sv.sparse_forms() == {"rows2"}
            assert sv.sparse_geometries() == ({want} if shared else {"per_wave"})
    assert np.isfinite(out[1]).all() and np.isfinite(out[0]).all()
    diff = np.abs(out[1] - out[0]).max()
    print(f"B = {B}: {want}, max |E - E(per-wave geometry)| over all {B} = {diff:.3e} (bound {1e-12 * case.scale:.3e})")
    assert diff < 1e-12 * case.scale
    return out[1]


@pytest.mark.parametrize("B", [T, T + 1, T + 5, T + 7, 8192 + 3, 5 * 8192 + 6])
def test_h2o_against_the_per_wave_geometry(testing_lib, h2o, B):
    """whole work items, tails of 1, 5, 7, 3 and 6 evaluations; 5121 work items: every grid wraps (at most 256 CUs x 8 workgroups)"""
    _both_geometries(h2o, B, 7000 + B, H2O_GEOMETRY)


@pytest.mark.parametrize("B", [T, T + 2, T + 7, 3 * 8192 + 4])
def test_lih_against_the_per_wave_geometry(testing_lib, lih, B):
    """the second instance: tails of 2, 7 and 4 evaluations; 3073 work items: every grid wraps"""
    _both_geometries(lih, B, 9000 + B, LIH_GEOMETRY)


@pytest.mark.parametrize("mol", ["h2o", "lih"])
def test_program_info_names_the_pieces(gpu_lib, request, mol):
    from openvqe_amd.backend import Statevector
    case = request.getfixturevalue(mol)
    rpt, epr = H2O_SHAPE if mol == "h2o" else LIH_SHAPE
    with Statevector(case.n) as sv:
        sv.set_hamiltonian(case.H)
        case.program(sv)
        sv.energy_batch(np.zeros((2, case.K)))
        info = sv.program_info()
    assert info["sp_h_slots"] == rpt * epr
    assert info["sp_h_reads_per_state"] == rpt * (epr + 1)
    assert -(-info["sp_h_entries"] // epr) <= info["sp_h_pieces"] <= NT * rpt
    assert info["sp_h_reads_per_state"] < 2 * -(-info["sp_h_entries"] // NT)      # fewer reads than two per entry


def test_entries_that_do_not_pack_stay_on_the_per_wave_geometry(testing_lib, h2o):
    """the selection is "the instance's criterion as before AND the packer succeeded": with the packer's answer forced to "does not
    fit" the same program and batch run k_sparse_vqe_rows<2>, and the energies are those of the workgroup geometry"""
    from openvqe_amd.backend import Statevector
    B = T + 3
    rng = np.random.default_rng(5)
    th = rng.uniform(-1, 1, (B, h2o.K))
    with Statevector(h2o.n) as sv:
        sv.set_option("sparse_pack", 0)
        sv.set_hamiltonian(h2o.H)
        h2o.program(sv)
        e0 = sv.energy_batch(th)
        assert sv.sparse_forms() == {"rows2"} and sv.sparse_geometries() == {"per_wave"}
        info = sv.program_info()
        assert info["sp_h_pieces"] == 0 and info["sp_h_slots"] == 0 and info["sp_h_reads_per_state"] == 0
        sv.set_option("sparse_pack", 1)
        e1 = sv.energy_batch(th)
        assert sv.sparse_geometries() == {"per_wave", H2O_GEOMETRY}
        assert sv.program_info()["sp_h_pieces"] > 0
    assert np.abs(e1 - e0).max() < 1e-12 * h2o.scale
