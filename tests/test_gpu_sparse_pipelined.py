"""The pipelined item loop of the workgroup geometry of the rows form (k_sparse_vqe_rows_shared, sv_sparse.hpp): table records held
in registers for the launch, the next item's theta loads in flight across the contraction, its cos/sin table written before the
second barrier, row words carried from item to item.

Only the FIRST item of a workgroup builds its table with nothing in front of it; every later one is prepared behind the item before.
So the tests move parameter vectors between first and later items (and between waves) and ask for the same bits, at the shapes
where the loop takes another path: a table beyond the records a lane holds (32 TE angles: 160 on the H2O instance, 96 on LiH),
a table of fewer angles than lanes, and angles on both sides of the large-argument branch of sincos inside one work item."""
import numpy as np
import pytest

from tests.test_gpu_sparse import Case, _designed, _thetas_with_nan_tail, h2o, testing_lib  # noqa: F401
from tests.test_gpu_sparse_shared import H2O_GEOMETRY, LIH_GEOMETRY, _device_batch, _sample_shared, lih  # noqa: F401
from tests.util import cascade_geometry

pytestmark = pytest.mark.gpu

B3 = 3 * 4096 + 5     # 1537 work items of 8, the last one partial: every workgroup of a grid of 512 (two per CU on 256 CUs: the H2O
                      # instance) walks at least three, of a grid of 768 (three per CU: LiH) at least two
SHIFT = 4096 + 24     # 515 work items: first <-> later items of a workgroup on either grid, other workgroups, other waves


def _two_layers(case):
    """the same generators twice, the second layer on parameters of its own: twice the distinct angles on the same support and
    the same restricted Hamiltonian"""
    cat = np.concatenate
    return Case(case.n, case.hf, cat([case.rx, case.rx]), cat([case.rz, case.rz]), cat([case.rc, case.rc]),
                cat([case.rp, case.rp + case.K]), 2 * case.K, case.H)


def _shifted_twice(case, full, B, geometry, oracle=True):
    """full[:B] and the same rows shifted cyclically by SHIFT, both with NaN rows behind the batch into a NaN-filled output:
    the energies move with their rows bit for bit, the output tail keeps its bits, a sample agrees with the C oracle"""
    from openvqe_amd.backend import Statevector
    shifted = np.ascontiguousarray(np.concatenate([np.roll(full[:B], SHIFT, axis=0), full[B:]]))
    with Statevector(case.n) as sv:
        sv.set_hamiltonian(case.H)
        case.program(sv)
        e, tail_kept = _device_batch(sv, full, B)
        e_shift, tail_kept_shift = _device_batch(sv, shifted, B)
        assert sv.sparse_forms() == {"rows2"}
        assert sv.sparse_geometries() == {geometry}
    assert tail_kept and tail_kept_shift
    assert np.isfinite(e).all()
    moved = np.flatnonzero(np.roll(e, SHIFT).view(np.int64) != e_shift.view(np.int64))
    print(f"B = {B}: {geometry}, energies whose bits changed under the shift: {moved.size}")
    assert moved.size == 0, moved[:16]
    if oracle:
        idx = _sample_shared(B)
        err = np.abs(e[idx] - case.oracle(full[idx])).max()
        print(f"B = {B}: max |E - oracle| on {idx.size} samples = {err:.3e} (bound {1e-11 * case.scale:.3e})")
        assert err < 1e-11 * case.scale
    return e


@pytest.mark.parametrize("mol", ["H2O", "LiH"])
def test_first_item_against_later_items_bit_for_bit(gpu_lib, h2o, lih, mol):
    case, geometry = (h2o, H2O_GEOMETRY) if mol == "H2O" else (lih, LIH_GEOMETRY)
    full = _thetas_with_nan_tail(np.random.default_rng(31), B3, case.K, extra=64)
    _shifted_twice(case, full, B3, geometry)


@pytest.mark.parametrize("mol", ["H2O", "LiH"])
def test_more_angles_than_a_lane_holds_records(gpu_lib, h2o, lih, mol):
    """two UCCSD layers: 280 distinct angles on the H2O instance (160 in registers), 184 on LiH (96) — the same instances take
    them (H2O: 8 x (4104 + 281 x 16) + 256 bytes of LDS, about 69 KB), the entries past the records load theirs at sincos time"""
    from openvqe_amd.backend import Statevector
    base, geometry = (h2o, H2O_GEOMETRY) if mol == "H2O" else (lih, LIH_GEOMETRY)
    case = _two_layers(base)
    with Statevector(case.n) as sv:
        sv.set_hamiltonian(case.H)
        case.program(sv)
        sv.energy_batch(np.zeros((2, case.K)))
        info = sv.program_info()
    assert info["support"] == (441 if mol == "H2O" else 225)
    full = _thetas_with_nan_tail(np.random.default_rng(32), B3, case.K, scale=0.3, extra=64)
    _shifted_twice(case, full, B3, geometry)


def test_fewer_angles_than_lanes(gpu_lib):
    """128 basis states, 7 angles: lanes 7..31 of every half-wave hold no record of their own and write nothing"""
    from openvqe_amd.backend import Statevector
    n, hf, gens, K = cascade_geometry(5, 0, 2)
    assert K < 32
    case = _designed(n, hf, gens, K, seed=128)
    B = 2048 + 3
    full = _thetas_with_nan_tail(np.random.default_rng(33), B, case.K, scale=2.0, extra=64)
    with Statevector(case.n) as sv:
        sv.set_hamiltonian(case.H)
        case.program(sv)
        e, tail_kept = _device_batch(sv, full, B)
        assert sv.sparse_forms() == {"rows2"}
        assert sv.sparse_geometries() == {LIH_GEOMETRY}
        assert sv.program_info()["support"] == 128
    assert tail_kept
    assert np.isfinite(e).all()
    idx = _sample_shared(B)
    err = np.abs(e[idx] - case.oracle(full[idx])).max()
    print(f"B = {B}: max |E - oracle| on {idx.size} samples = {err:.3e} (bound {1e-11 * case.scale:.3e})")
    assert err < 1e-11 * case.scale


def test_large_and_small_angles_inside_one_work_item(gpu_lib, h2o):
    """theta = +- (1 + j / 8) 2^k, j < 8, k = -7 .. 34, drawn per element: sincos branches to its large-argument reduction at
    |x| >= 2^30, and whatever power of two between 1/8 and 1 multiplies a parameter in the table, products on both sides of it meet
    in every parameter row, so in every work item and half-wave.  Four significant bits: coeff * theta is exact in the kernel and
    in the oracle, which rotates string by string — the comparison is of sincos alone and keeps the bound of the other tests."""
    rng = np.random.default_rng(34)
    full = _thetas_with_nan_tail(rng, B3, h2o.K, extra=64)
    k = rng.integers(-7, 35, (B3, h2o.K))
    rows = np.arange(B3)
    k[rows, rng.integers(0, h2o.K // 2, B3)] = 34                # (in every row for certain, not only almost surely)
    k[rows, rng.integers(h2o.K // 2, h2o.K, B3)] = -7
    full[:B3] = rng.choice([-1.0, 1.0], (B3, h2o.K)) * (1.0 + rng.integers(0, 8, (B3, h2o.K)) / 8.0) * np.exp2(k)
    assert ((k >= 33).any(axis=1) & (k <= 0).any(axis=1)).all()
    _shifted_twice(h2o, full, B3, H2O_GEOMETRY)
