"""CPU tests of ``ShardedStatevector.ground_state`` / ``PartitionedStatevector.ground_state``: world size 2 and 4 over gloo, the
shard arithmetic by the oracle-backed engine (complex storage, the vector operations by the torch fall-back), so that the
recurrence, its collectives and the buffer rotation are exercised without GPUs — a real-symmetric molecular Hamiltonian and a
complex Hermitian one with odd-Y strings, several chunks per partner read."""
import pytest

from tests.lanczos_cases import check_ranks, run_ranks


@pytest.mark.parametrize("world,chunk_bits,kind,args", [
    (2, 5, "molecule", (4, 2, 2)),          # 8 qubits: shards of 2^7, four chunks per partner read
    (4, 4, "molecule", (4, 2, 1)),          # two rank bits
    (2, None, "odd_y", (8, 11)),            # complex Hermitian, default chunks
    (4, 4, "odd_y", (9, 12)),
])
def test_ground_state_on_cpu_shards(world, chunk_bits, kind, args):
    r0 = check_ranks(run_ranks(world, "oracle", chunk_bits, kind, args), kind, args)
    assert not r0["stored_real"] and not r0["flagged_real"]      # the CPU engine offers no float64 shards
