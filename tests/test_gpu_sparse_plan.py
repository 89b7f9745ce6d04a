"""The tables of the host planner (openvqe_amd/csrc/sparse_plan.hpp: numbering, orientation, lanes and pads of the rows of 32;
sparse_pack.hpp: slot order of the owner pieces) under the two kernels that walk them: the throughput form in its workgroup
geometry (k_sparse_vqe_rows_shared, taken from 2048 evaluations on when an instance holds the program) and the per-wave form
k_sparse_vqe_rows<2> (testing option "sparse_shared" = 0), which reads the same rows.

Programs: LiH (12 qubits) and H2O (14 qubits) STO-3G UCCSD, and the designed programs of tests/test_sparse_plan.py whose ops have
1, 15, 16, 17, 31, 32, 33, 64 and 65 pairs (8 and 9 qubits).  Batches: 2048, the smallest that selects the form, and 2053, whose last
work item of 8 (2) evaluations is partly empty.  Angles of both signs.  Energies against the C oracle within the bound of
tests/test_gpu_sparse.py, identical bits from two launches and under a cyclic shift of the batch."""
import numpy as np
import pytest

from tests.test_gpu_sparse import Case, _designed, _sample, _thetas_with_nan_tail, h2o, testing_lib  # noqa: F401
from tests.test_gpu_sparse_shared import H2O_GEOMETRY, LIH_GEOMETRY, T, lih  # noqa: F401
from tests.test_sparse_plan import PARENT, designed_generators

pytestmark = pytest.mark.gpu

SHARED = {H2O_GEOMETRY, LIH_GEOMETRY}


def _run(case, B, seed, shared, scale=1.0):
    from openvqe_amd.backend import Statevector
    rng = np.random.default_rng(seed)
    full = _thetas_with_nan_tail(rng, B, case.K, scale=scale)
    th = np.ascontiguousarray(full[:B])
    assert (th < 0).any() and (th > 0).any()
    shifted = np.ascontiguousarray(np.roll(th, 3, axis=0))
    with Statevector(case.n) as sv:
        if not shared:
            sv.set_option("sparse_shared", 0)
        sv.set_hamiltonian(case.H)
        case.program(sv)
        e1 = sv.energy_batch(th)
        e2 = sv.energy_batch(th)
        e3 = sv.energy_batch(shifted)
        assert sv.sparse_forms() == {"rows2"}
        geometries = sv.sparse_geometries()
        info = sv.program_info()
    assert np.isfinite(e1).all()
    idx = np.array(sorted(set(int(i) for i in _sample(B)) | set(range(B - 10, B))))
    err = np.abs(e1[idx] - case.oracle(th[idx])).max()
    print(f"B = {B}: {sorted(geometries)}, max |E - oracle| on {idx.size} samples = {err:.3e} (bound {1e-11 * case.scale:.3e}); "
          f"LDS cycles per evaluation: rows {info['sp_lds_row_reads']} + {info['sp_lds_row_writes']}, <H> {info['sp_lds_h_reads']}; "
          f"discovery order {info['sp_lds_row_reads_discovery_order']} + {info['sp_lds_row_writes_discovery_order']}")
    assert err < 1e-11 * case.scale
    assert np.array_equal(e1.view(np.int64), e2.view(np.int64))
    assert np.array_equal(np.roll(e1, 3).view(np.int64), e3.view(np.int64))
    return geometries, info


@pytest.mark.parametrize("B", [T, T + 5])
@pytest.mark.parametrize("shared", [True, False])
def test_h2o(testing_lib, h2o, shared, B):
    geometries, info = _run(h2o, B, 14 + B, shared)
    assert geometries == ({H2O_GEOMETRY} if shared else {"per_wave"})
    # the report (ovqe_program_info [33..37]) against the tables of the planner before this one (tests/test_sparse_plan.py)
    got = (info["sp_lds_row_reads"], info["sp_lds_row_writes"], info["sp_lds_h_reads"])
    assert all(0 < g <= p for g, p in zip(got, PARENT["H2O"])), got
    assert sum(got) <= 0.75 * sum(PARENT["H2O"])
    assert got[0] <= info["sp_lds_row_reads_discovery_order"] and got[1] <= info["sp_lds_row_writes_discovery_order"]


@pytest.mark.parametrize("B", [T, T + 5])
@pytest.mark.parametrize("shared", [True, False])
def test_lih(testing_lib, lih, shared, B):
    geometries, info = _run(lih, B, 12 + B, shared)
    assert geometries == ({LIH_GEOMETRY} if shared else {"per_wave"})
    got = (info["sp_lds_row_reads"], info["sp_lds_row_writes"], info["sp_lds_h_reads"])
    assert all(0 < g <= p for g, p in zip(got, PARENT["LiH"])), got


@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("s", [15, 17, 31, 33, 64, 65])
def test_designed_pair_counts(testing_lib, s, shared):
    """an op of s pairs: 32 - s % 32 padded lanes, the halves of 16 on both sides of their boundary, ops of more than one row
    (64: Y rotations on bits 1..7, ops of 1, 2, 4, 8, 16, 32 and 64 pairs — the program of s = 1, 16 and 32 as well)"""
    n, hf, gens, K = designed_generators(s)
    case = _designed(n, hf, gens, K, seed=s)
    for B in (T, T + 5):
        geometries, info = _run(case, B, 100 * s + B, shared, scale=2.0)
        assert info["support"] > 32 and info["sp_conflicts"] <= info["sp_conflicts_discovery_order"]
        if shared:
            # (the workgroup geometry when an instance holds the program's entries: sparse_host.inc)
            assert geometries == ({"per_wave"} if info["sp_h_pieces"] == 0 else geometries & SHARED) and geometries
        else:
            assert geometries == {"per_wave"}
