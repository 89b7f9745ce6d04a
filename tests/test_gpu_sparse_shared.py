"""The workgroup geometry of the rows form (k_sparse_vqe_rows_shared, sv_sparse.hpp: four waves per workgroup, two evaluations per
wave, the restricted Hamiltonian's entries in registers for the whole launch) against the C oracle, against the per-wave
geometry (k_sparse_vqe_rows<2>) and against itself bit for bit.

run_sparse picks it for batches of at least T evaluations when an instance holds the program; both geometries report the form
"rows2", ``Statevector.sparse_geometries()`` names the one that ran.  Work items are 2 NW = 8 evaluations: batches of every kind
of residue mod 8 are run with NaN parameter rows behind the batch and a NaN-filled output that must keep its tail."""
import numpy as np
import pytest

from tests.test_gpu_sparse import (Case, _check_batch, _designed, _form_for, _sample, _thetas_with_nan_tail, h2o,  # noqa: F401
                                   testing_lib)
from tests.util import cascade_geometry

pytestmark = pytest.mark.gpu

T = 2048             # sparse_host.inc: SHARED_MIN_B (= the smallest batch of the rows form: below it "plain1" runs)
NS = 8               # evaluations per work item
H2O_GEOMETRY = "shared_e37_s4104"
LIH_GEOMETRY = "shared_e13_s2568"


def _sample_shared(B):
    """the sample of the existing helper + both sides of every multiple of 4096 evaluations (the persistent grid is a multiple of
    256 workgroups of 8 evaluations wherever the chip has a multiple of 256 CUs / 2 workgroups per CU) + the last work item"""
    idx = set(int(i) for i in _sample(B))
    for w in range(4096, B + 1, 4096):
        idx.update({w - NS, w - 1, w, w + NS - 1})
    idx.update(range(B - B % NS - NS, B))
    return np.array(sorted(i for i in idx if 0 <= i < B))


def _device_batch(sv, full, B):
    """energies of full[:B] through the device entry point into a NaN-filled tensor of B + 64: -> (energies, the tail kept its bits)"""
    import torch
    th_dev = torch.from_numpy(full).cuda()
    en = torch.full((B + 64,), float("nan"), dtype=torch.float64, device="cuda")
    tail_bits = en[B:].view(torch.int64).cpu().clone()
    sv.energy_batch_device(B, th_dev.data_ptr(), en.data_ptr())
    torch.cuda.synchronize()
    return en[:B].cpu().numpy(), torch.equal(en[B:].view(torch.int64).cpu(), tail_bits)


def _run_and_compare(case, B, seed, want, lib_options=True):
    """the batch on a handle that sets no option (device entry point), the oracle on the sample, and every energy against the
    per-wave geometry (testing option "sparse_shared" = 0).  want = None: a batch below the rows form (no geometry reported)"""
    from openvqe_amd.backend import Statevector
    rng = np.random.default_rng(seed)
    full = _thetas_with_nan_tail(rng, B, case.K, extra=64)
    with Statevector(case.n) as sv:
        sv.set_hamiltonian(case.H)
        case.program(sv)
        e, tail_kept = _device_batch(sv, full, B)
        assert sv.sparse_forms() == {"rows2" if want else _form_for(B)}
        assert sv.sparse_geometries() == ({want} if want else set())
    assert tail_kept
    assert np.isfinite(e).all()
    idx = _sample_shared(B)
    ref = case.oracle(full[idx])
    err = np.abs(e[idx] - ref).max()
    print(f"B = {B}: {want}, max |E - oracle| on {idx.size} samples = {err:.3e} (bound {1e-11 * case.scale:.3e})")
    assert err < 1e-11 * case.scale
    if lib_options:
        with Statevector(case.n) as sv:
            sv.set_option("sparse_shared", 0)
            sv.set_hamiltonian(case.H)
            case.program(sv)
            e_wave = sv.energy_batch(full[:B])
            assert sv.sparse_forms() == {"rows2" if want else _form_for(B)}
            assert sv.sparse_geometries() == ({"per_wave"} if want else set())
        diff = np.abs(e - e_wave).max()
        print(f"B = {B}: max |E - E(per-wave geometry)| over all {B} = {diff:.3e} (bound {1e-12 * case.scale:.3e})")
        assert diff < 1e-12 * case.scale
    return e


@pytest.mark.parametrize("B", [T - 1, T, T + 1, T + 3, T + 6, T + 7, 5 * 8192 + 5])
def test_headline_workload_threshold_tails_and_wrap(testing_lib, h2o, B):
    """H2O/STO-3G UCCSD at both sides of the batch threshold (below it: one evaluation per wave, no rows form), batches that are
    1, 3, 6, 7 and 5 past a multiple of 8 (the last work item holds fewer than 8 evaluations: its spare states run the clamped
    last row, nothing is stored for them) and a batch of 5121 work items (every grid wraps)"""
    _run_and_compare(h2o, B, B, None if B < T else H2O_GEOMETRY)


def test_same_bits_twice_from_both_entry_points_and_under_row_permutation(gpu_lib, h2o):
    """the energy of a parameter vector depends neither on the run, nor on the entry point, nor on the work item, wave or half-wave
    that evaluated it (this also catches any cross-talk between the states of a workgroup).  Product library, no option."""
    from openvqe_amd.backend import Statevector
    B = max(T, 16384) + 5
    rng = np.random.default_rng(99)
    full = _thetas_with_nan_tail(rng, B, h2o.K, extra=64)
    perm = rng.permutation(B)
    permuted = np.ascontiguousarray(np.concatenate([full[:B][perm], full[B:]]))
    with Statevector(h2o.n) as sv:
        sv.set_hamiltonian(h2o.H)
        h2o.program(sv)
        e1 = sv.energy_batch(full[:B])
        e2 = sv.energy_batch(full[:B])
        e_dev, tail_kept = _device_batch(sv, full, B)
        e_perm, tail_kept_p = _device_batch(sv, permuted, B)
        assert sv.sparse_forms() == {"rows2"}
        assert sv.sparse_geometries() == {H2O_GEOMETRY}
    assert tail_kept and tail_kept_p
    assert np.array_equal(e1.view(np.int64), e2.view(np.int64))
    assert np.array_equal(e1.view(np.int64), e_dev.view(np.int64))
    assert np.array_equal(e1[perm].view(np.int64), e_perm.view(np.int64))
    idx = _sample_shared(B)
    assert np.abs(e1[idx] - h2o.oracle(full[idx])).max() < 1e-11 * h2o.scale


@pytest.fixture(scope="module")
def lih(gpu_lib):
    """LiH/STO-3G UCCSD: 225 of 4096 amplitudes (256 slots + 64 spare: 2560 bytes, a stride of 2568), 92 parameters"""
    from openvqe_amd import chem, fermion
    from openvqe_amd.backend import compile_ucc_program
    mol = chem.molecule("LiH")
    mol.rhf()
    ham, hf = mol.jw_hamiltonian(), mol.hf_init()
    gens = fermion.uccsd_generators(mol.nao, mol.n_elec // 2)
    n = ham.nbqbits
    rx, rz, rc, rp, K = compile_ucc_program(n, gens)
    hf_index = int(sum(1 << (n - 1 - q) for q, v in enumerate(hf) if v)) if not np.isscalar(hf) else int(hf)
    return Case(n, hf_index, rx, rz, rc, rp, K, ham)


def test_second_instance_lih(testing_lib, lih):
    """a program of another stride and entry count takes the second instance"""
    from openvqe_amd.backend import Statevector
    with Statevector(lih.n) as sv:
        sv.set_hamiltonian(lih.H)
        lih.program(sv)
        sv.energy_batch(np.zeros((2, lih.K)))
        info = sv.program_info()
    assert info["support"] == 225
    assert info["sp_h_entries"] <= 256 * 13, info["sp_h_entries"]
    _run_and_compare(lih, 8192 + 11, 12, LIH_GEOMETRY)   # (1026 work items: more than four workgroups on each of 256 CUs)


def test_second_instance_in_the_product_library(gpu_lib, lih):
    """... and is launched by the product library too (no option anywhere), at a batch of whole work items"""
    _run_and_compare(lih, T + 8, 13, LIH_GEOMETRY, lib_options=False)


def test_support_beyond_every_stride_stays_on_the_per_wave_geometry(gpu_lib):
    """1024 basis states (8704 bytes per state with the spare slots) at B >= T: "rows2" on one wave per pair of evaluations,
    8194 work items on a grid of 8192"""
    from openvqe_amd.backend import Statevector
    n, hf, gens, K = cascade_geometry(10, 0, 0)
    case = _designed(n, hf, gens, K, seed=1024)
    B = 16387
    rng = np.random.default_rng(1024)
    full = _thetas_with_nan_tail(rng, B, case.K, scale=2.0)
    with Statevector(case.n) as sv:
        sv.set_hamiltonian(case.H)
        case.program(sv)
        e = sv.energy_batch(full[:B])
        assert sv.sparse_forms() == {"rows2"}
        assert sv.sparse_geometries() == {"per_wave"}
        assert sv.program_info()["support"] == 1024
        _check_batch(case, sv, full[:B], e)
