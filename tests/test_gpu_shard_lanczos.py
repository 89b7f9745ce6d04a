"""``PartitionedStatevector.ground_state`` on HIP shards at world size 2, 4 and 8 (one process per rank over gloo, every shard handle
on device 0): the Jordan-Wigner Hamiltonian of a 12-qubit synthetic molecule, real-symmetric, so the recurrence runs on float64
shards — sigma = H psi by the real APPLY kernels (k_tile_cross_real / k_cross_small_real, the d = 0 groups through the same kernels),
the vector operations by ovqe_vec_*, the start vector by the real fill of ovqe_randomize.  Against the ARPACK oracle and against
the one-device ``Statevector.ground_state``."""
import pytest

from tests.lanczos_cases import check_ranks, reference, run_ranks

pytestmark = pytest.mark.gpu

MOLECULE = (6, 3, 1)


@pytest.fixture(scope="module")
def one_device(gpu_lib):
    from openvqe_amd.backend import Statevector
    ham, _, _ = reference("molecule", *MOLECULE)
    with Statevector(ham.nbqbits) as sv:
        sv.set_hamiltonian(ham)
        return sv.ground_state(tol=1e-10, max_iter=3000)


@pytest.mark.parametrize("world,chunk_bits,tile_bits,small", [
    (2, 11, 11, 0),      # shards of 2^11 doubles read in one chunk: the real tile form across shards and inside them
    (2, 8, 0, 1),        # chunks below the tile sizes: the small form across shards, tiles inside
    (4, 7, 0, 1),        # shards of 2^10: the small form everywhere, two rank bits
    (8, 6, 0, 1),        # three rank bits, seven partners
])
def test_ground_state_on_hip_shards(gpu_lib, one_device, world, chunk_bits, tile_bits, small):
    r0 = check_ranks(run_ranks(world, "hip", chunk_bits, "molecule", MOLECULE), "molecule", MOLECULE)
    assert r0["stored_real"] and r0["flagged_real"]                       # float64 shards: engine.is_real
    assert r0["info"]["tile_bits"] == tile_bits and r0["info"]["streaming_fallback"] == small
    assert abs(r0["e"] - one_device[0]) < 1e-9
