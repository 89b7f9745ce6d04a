"""k-bit shard exchanges on the GPU: the pack / unpack kernels alone (ovqe_shard_pack / ovqe_shard_unpack through
backend.Statevector: copies, so every comparison is bit for bit), then the workers of tests/test_exchange_multibit.py on HIP shards
at world size 4 and 8 (every rank's shard on device 0, gloo), a PartitionedStatevector energy against the oracle engine, and a dry
rank of an 8-rank register."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _block_index(n_local, mask, block):
    """shard positions of block ``block`` of the local bits ``mask``, in ascending order"""
    j = np.arange(1 << (n_local - bin(mask).count("1")), dtype=np.int64)
    out, i, src = np.zeros_like(j), 0, 0
    for bit in range(n_local):
        if (mask >> bit) & 1:
            out |= ((block >> i) & 1) << bit
            i += 1
        else:
            out |= ((j >> src) & 1) << bit
            src += 1
    return out


def _masks(n_local, rng):
    top = n_local - 1
    fixed = [0b1, 0b10, 0b11, 0b101, 0b111, 0b110, 1 << top, 0b11 << (top - 1), 0b111 << (top - 2), (1 << top) | 1, (1 << top) | 0b10,
             (1 << top) | (1 << (n_local // 2)) | 1, 0b11 << (n_local // 2), (1 << (n_local // 2)) | (1 << (n_local // 2 + 2)), 0b11011]
    drawn = [sum(1 << int(b) for b in rng.choice(n_local, k, replace=False)) for k in (1, 2, 3, 3, 4, 6)]
    return fixed + drawn


@pytest.mark.parametrize("n_local", [10, 13, 16, 20])
@pytest.mark.parametrize("storage", ["complex", "real_state", "real_parts_only"])
def test_pack_and_unpack_kernels_are_exact_copies(gpu_lib, n_local, storage):
    import torch
    from openvqe_amd.backend import Statevector
    rng = np.random.default_rng(100 * n_local + len(storage))
    size = 1 << n_local
    real_state, rpo = storage == "real_state", storage == "real_parts_only"
    host = rng.normal(size=size) if real_state else rng.normal(size=size) + 1j * rng.normal(size=size)
    state = torch.from_numpy(host).cuda()
    zero = torch.zeros_like(state)
    stream_dtype = torch.complex128 if storage == "complex" else torch.float64
    with Statevector(n_local) as sv, Statevector(n_local) as sv0:
        sv.adopt_state(state.data_ptr())
        sv0.adopt_state(zero.data_ptr())
        if real_state:
            sv.set_option("real_state", 1)
            sv0.set_option("real_state", 1)
        cases = 0
        for mask in _masks(n_local, rng):
            k = bin(mask).count("1")
            bsize = size >> k
            blocks = range(1 << k) if k <= 3 else [0, (1 << k) - 1, int(rng.integers(0, 1 << k))]
            for block in blocks:
                idx = _block_index(n_local, mask, block)
                want = host[idx].real if rpo else host[idx]
                # whole block, then uneven pieces (odd boundaries: the 8-byte paths; an odd offset into the buffer too)
                cuts = sorted({0, bsize} | {int(c) for c in rng.integers(0, bsize + 1, 3)} | {1, bsize // 2})
                for ranges in ([(0, bsize)], list(zip(cuts, cuts[1:]))):
                    buf = torch.full((bsize + 1,), -7.0, dtype=stream_dtype, device="cuda")
                    off = 1 if (len(ranges) > 1 and storage != "complex") else 0
                    zero.zero_()
                    for a, b in ranges:
                        sv.shard_pack(mask, block, a, b - a, buf[off + a:].data_ptr(), rpo)
                    for a, b in ranges:
                        sv0.shard_unpack(mask, block, a, b - a, buf[off + a:].data_ptr(), rpo)
                    torch.cuda.synchronize()
                    got = buf.cpu().numpy()
                    assert np.array_equal(got[off:off + bsize], want), (mask, block, ranges)
                    assert np.all(got[:off] == -7.0) and np.all(got[off + bsize:] == -7.0)      # nothing beyond the range written
                    back = zero.cpu().numpy()
                    expect = np.zeros_like(host)
                    expect[idx] = want                     # (real parts only: the imaginary parts are exact zeros)
                    assert np.array_equal(back, expect), (mask, block, ranges)
                    cases += 1
        torch.cuda.synchronize()
        assert np.array_equal(state.cpu().numpy(), host)          # pack never writes the shard
        assert cases >= 100


def test_pack_and_unpack_refuse_bad_arguments(gpu_lib):
    import torch
    from openvqe_amd._lib import BackendError
    from openvqe_amd.backend import Statevector
    n_local = 10
    host = np.arange(1 << n_local) + 1j
    state = torch.from_numpy(host).cuda()
    buf = torch.full((1 << n_local,), 5.0, dtype=torch.complex128, device="cuda")
    with Statevector(n_local) as sv:
        sv.adopt_state(state.data_ptr())
        for call in (sv.shard_pack, sv.shard_unpack):
            for args, text in (((1 << n_local, 0, 0, 1), "local bits"), ((0, 0, 0, 1), "local bits"), ((0b1111111, 0, 0, 1), "local bits"),
                               ((0b11, 4, 0, 1), "block value"), ((0b11, 1, 0, 257), "range past"), ((0b11, 1, 200, 57), "range past"),
                               ((0b11, 1, -1, 2), "range past"), ((0b11, 1, 0, -1), "range past")):
                with pytest.raises(BackendError, match=text):
                    call(*args, buf.data_ptr())
            with pytest.raises(BackendError, match="null buffer"):
                call(0b11, 1, 0, 4, 0)
            with pytest.raises(BackendError, match="aligned"):
                call(0b11, 1, 0, 4, buf.data_ptr() + 8)
            call(0b11, 1, 256, 0, buf.data_ptr())              # an empty range at the end of the block is no error
        torch.cuda.synchronize()
        assert np.array_equal(state.cpu().numpy(), host) and np.all(buf.cpu().numpy() == 5.0)
        sv.shard_pack(0b11, 1, 0, 256, buf.data_ptr())          # ... and the handle still works
        torch.cuda.synchronize()
        assert np.array_equal(buf.cpu().numpy()[:256], host[1::4])


@pytest.mark.parametrize("world,n", [(4, 15), (8, 16), (8, 15)])
def test_multibit_exchange_on_hip_shards(gpu_lib, world, n):
    from tests.test_exchange_multibit import check_exchange_results, launch
    seed = 900 + 10 * world + n
    check_exchange_results(launch(world, n, seed, engine="hip", timeout=600), world, n, seed, hip=True)


def _partitioned_worker(rank, world, port, out):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from openvqe_amd import fermion, partitioned
        from tests.test_distributed import OracleShardEngine
        ham, gens, hf = fermion.synthetic_molecule(7, 1, 11)          # 14 qubits; the occupied orbitals sit on the rank bits
        rng = np.random.default_rng(3)
        thetas = rng.uniform(-0.3, 0.3, (2, len(gens)))
        res = {}
        for engine in ("hip", "oracle"):
            partitioned.ENGINE_FACTORY = OracleShardEngine if engine == "oracle" else None
            with partitioned.PartitionedStatevector(14, device=0) as sv:
                sv.set_hamiltonian(ham)
                sv.set_ucc_program(gens, hf)
                res[engine] = ([sv.energy(t) for t in thetas], sv.program_info(), dict(sv.sharded.stats))
        if rank == 0:
            out.put(res)
    finally:
        dist.destroy_process_group()


def test_partitioned_ucc_energy_through_multibit_exchanges(gpu_lib):
    import torch.multiprocessing as mp
    from tests.test_distributed import _free_port
    world = 4
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_partitioned_worker, args=(r, world, port, out)) for r in range(world)]
    for p in procs:
        p.start()
    res = out.get(timeout=600)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    (e_hip, info, st), (e_cpu, info_cpu, st_cpu) = res["hip"], res["oracle"]
    assert np.abs(np.array(e_hip) - np.array(e_cpu)).max() < 1e-11
    assert info["exchange_bits"] > info["exchanges"] >= 1 and info["exchange_bits"] == info_cpu["exchange_bits"]
    assert st["exchange_bits"] == 2 * info["exchange_bits"] and st["swaps"] == 2 * info["exchanges"]       # two evaluations
    # (UCC generators keep the state real: float64 shards on the HIP engine, real parts on the wire of the oracle engine — 8 bytes each)
    assert st["real_exchanges"] == st["swaps"] and st["link_bytes"] == st_cpu["link_bytes"] and st["bytes_sent"] == st_cpu["bytes_sent"]


@pytest.mark.parametrize("storage", ["complex", "real_parts", "float64"])
def test_dry_rank_runs_a_three_bit_exchange_with_the_real_ranks_byte_counts(gpu_lib, storage):
    """one rank of an 8-rank register alone: packs, "receives" its own pieces and unpacks for all seven partners — the shard is
    unchanged, 7/8 of it is counted as sent and 1/8 on the busiest link"""
    import torch
    from openvqe_amd.distributed import ShardedStatevector
    n, nl = 19, 16
    sv = ShardedStatevector(n, device=0, dry_rank=(8, 3))
    sv.randomize(7)
    if storage == "float64":
        sv.engine.set_real(True)
    sv.real = storage != "complex"
    if storage == "real_parts":
        sv.engine.tensor.copy_(torch.complex(sv.engine.tensor.real, torch.zeros_like(sv.engine.tensor.real)))
    before = sv.engine.tensor.clone()
    ebytes = 16 if storage == "complex" else 8
    sv._swap_bits([nl, nl + 1, nl + 2], [2, 9, 0])
    assert torch.equal(sv.engine.tensor, before) and sv.engine.tensor.dtype == before.dtype
    assert sv.stats["swaps"] == 1 and sv.stats["exchange_bits"] == 3 and sv.stats["pieces"] == sv.EXCHANGE_PIECES
    assert sv.stats["bytes_sent"] == 7 * (ebytes << nl) // 8 and sv.stats["link_bytes"] == (ebytes << nl) // 8
    sv._swap_bits([nl + 2, nl + 1, nl], [nl - 1, nl - 2, nl - 3])          # the top local bits: blocks sent from where they lie
    assert torch.equal(sv.engine.tensor, before)
    assert sv.stats["bytes_sent"] == 2 * 7 * (ebytes << nl) // 8 and sv.stats["link_bytes"] == 2 * (ebytes << nl) // 8
    assert sorted(sv.perm) == list(range(n))
