"""The planned ADAPT screen on HIP shards over gloo (one process per rank, every rank's shard handle on device 0): the screens of
tests/test_distributed.py through ovqe_xpool_*, the screen on float64 shards end to end, and one partitioned ADAPT flow through
PartitionedStatevector — each against the dense single-process formulas or the one-device handle."""
import os

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import masks
from tests.test_distributed import _free_port, _screen_worker

pytestmark = pytest.mark.gpu


def _spawn(target, world, args):
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, world, port) + tuple(args) + (out,)) for r in range(world)]
    for p in procs:
        p.start()
    res = out.get(timeout=600)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    return res


def _screen_entry(rank, world, port, n, seed, chunk_bits, out):
    _screen_worker(rank, world, port, n, seed, out, "hip", chunk_bits)


@pytest.mark.parametrize("world,n,chunk_bits", [(2, 15, 11), (4, 16, 12), (8, 16, 10)])
def test_planned_screen_on_hip_shards(gpu_lib, world, n, chunk_bits):
    """the fermionic and the qubit screen of one pool (tests/test_distributed.py _screen_worker) on HIP shards: tiles of 2^11, 2^12 and
    2^10 complex amplitudes for the partner chunks; ONE plan serves both screens"""
    gf, gq, stats, (xs, zs, phis, hx, hz, hc, pool, hf) = _spawn(_screen_entry, world, (n, 77 + n, chunk_bits))
    psi = np.zeros(1 << n, complex)
    psi[hf] = 1
    for x, z, p in zip(xs, zs, phis):
        psi = masks.rotate(psi, x, z, p)
    sigma = 0.3 * psi
    for x, z, c in zip(hx, hz, hc):
        sigma = sigma + c * masks.pauli_apply(psi, int(x), int(z))
    want = np.array([sum(c * np.vdot(sigma, masks.pauli_apply(psi, int(x), int(z))) for x, z, c in zip(*op)) for op in pool])
    print("max error fermionic %.3e qubit %.3e" % (np.abs(np.asarray(gf) - 2.0 * want.real).max(), np.abs(np.asarray(gq) - 2.0 * np.abs(want)).max()))
    assert np.abs(np.asarray(gf) - 2.0 * want.real).max() < 1e-11
    assert np.abs(np.asarray(gq) - 2.0 * np.abs(want)).max() < 1e-11
    assert stats["pool_plans"] == 1 and stats["screen_s"] > 0.0 and stats["full_shard_reads"] >= 2


def _odd_y_string(rng, n, weight=None):
    bits = [int(b) for b in rng.choice(n, int(rng.integers(2, 5)) if weight is None else weight, replace=False)]
    x = sum(1 << b for b in bits)
    return x, (1 << bits[0]) | (int(rng.integers(0, 1 << n)) & ~x)      # one Y, Z anywhere else


def _real_problem(n, seed, odd_y_in_h):
    rng = np.random.default_rng(seed)
    T = 24
    hx = [int(v) for v in rng.integers(0, 1 << n, T)]
    hx[:4] = [0, 0, 0, 0]
    hx[4] = 1 << (n - 1)
    hz = [int(v) for v in rng.integers(0, 1 << n, T)]
    hz = [z ^ (x & -x) if bin(x & z).count("1") & 1 else z for x, z in zip(hx, hz)]      # an even number of Y everywhere: real-symmetric
    hc = list(rng.normal(size=T))
    if odd_y_in_h:      # one string with an odd number of Y: H no longer maps real vectors to real vectors
        hx[7], hz[7] = _odd_y_string(rng, n)
    pool = []
    for _ in range(10):     # qubit-pool strings: an odd number of Y, coefficient +-1 (purely imaginary between real vectors)
        x, z = _odd_y_string(rng, n)
        pool.append(([x], [z], [complex(rng.choice([-1.0, 1.0]))]))
    for _ in range(10):     # two-term antisymmetric operators i/2 (P - Q), P and Q with an odd number of Y on the same x
        x, z = _odd_y_string(rng, n)
        bits = [b for b in range(n) if (x >> b) & 1]
        z2 = (z & ~x) | (1 << bits[1])
        pool.append(([x, x], [z, z2], [0.5j, -0.5j]))
    pool.append(([1 << (n - 1) | 1], [1], [1.0 + 0j]))     # x on the top rank bit
    # Y on every qubit (a dense product state: every matrix element of the screen is non-zero), then entangling odd-Y strings
    rots = [(1 << q, 1 << q) for q in range(n)] + [_odd_y_string(rng, n) for _ in range(6)]
    return hx, hz, hc, pool, rots, rng.uniform(0.3, 1.2, len(rots)), int(rng.integers(0, 1 << n))


def _real_worker(rank, world, port, n, seed, chunk_bits, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["OVQE_SHARD_CHUNK_BITS"] = str(chunk_bits)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from openvqe_amd.distributed import ShardedStatevector
        res = {}
        for label in ("ground", "program", "widened"):
            hx, hz, hc, pool, rots, phis, hf = _real_problem(n, seed, label == "widened")
            sv = ShardedStatevector(n, device=0)
            if label == "ground":
                sv.ground_state(hx, hz, hc, 0.0, tol=1e-3, max_iter=6)
            else:
                rx, rz = [r[0] for r in rots], [r[1] for r in rots]
                prog = sv.compile_program(rx, rz, np.ones(len(rots)), np.arange(len(rots)), hf)
                sv.run_program(prog, phis)
            before = sv._storage_real()
            reads0, real0 = sv.stats["chunk_reads"], sv.stats["real_chunk_reads"]
            gf = sv.pool_gradients((hx, hz, hc, 0.3), pool, "fermionic")
            after_first = sv._storage_real()
            gq = sv.pool_gradients((hx, hz, hc, 0.3), pool, "qubit")
            after = sv._storage_real() and after_first
            psi = np.asarray(sv.gather_state())      # (read back last: it widens a float64 shard; the screens leave the state as it was)
            res[label] = {"before": before, "after": after, "psi": psi, "gf": gf, "gq": gq,
                          "reads": sv.stats["chunk_reads"] - reads0, "real_reads": sv.stats["real_chunk_reads"] - real0,
                          "pool_plans": sv.engine.counters["pool_plans"], "sigma_dtype": str(sv._sigma.dtype),
                          "info": sv.engine.pool_info(next(iter(sv._pool_plans.values()))["pid"])}
            sv.free_pool_plans()
        if rank == 0:
            out.put(res)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,n,chunk_bits", [(2, 15, 11), (4, 16, 12)])
def test_screen_stays_on_float64_shards(gpu_lib, world, n, chunk_bits):
    """after ``ground_state`` of a real-symmetric H and after ``run_program`` of an odd-Y program the shard is float64, and
    ``pool_gradients`` leaves it so: sigma is a float64 buffer, the chunks travel as doubles (stats["real_chunk_reads"] grows by the
    chunks read), both gradient modes match the dense formulas to 1e-11.  With one string of H carrying an ODD number of Y — H then no
    longer maps real vectors to real vectors, the condition under which the screen may stay on doubles — the same call widens the
    shard and still matches."""
    res = _spawn(_real_worker, world, (n, 4000 + n, chunk_bits))
    for label in ("ground", "program", "widened"):
        hx, hz, hc, pool, _, _, _ = _real_problem(n, 4000 + n, label == "widened")
        r = res[label]
        psi = r["psi"]
        assert np.abs(psi.imag).max() == 0.0 and abs(np.vdot(psi, psi).real - 1.0) < 1e-10
        sigma = 0.3 * psi
        for x, z, c in zip(hx, hz, hc):
            sigma = sigma + c * masks.pauli_apply(psi, int(x), int(z))
        want = np.array([sum(c * np.vdot(sigma, masks.pauli_apply(psi, int(x), int(z))) for x, z, c in zip(*op)) for op in pool])
        print(label, "max error fermionic %.3e qubit %.3e" % (np.abs(r["gf"] - 2.0 * want.real).max(), np.abs(r["gq"] - 2.0 * np.abs(want)).max()))
        assert np.abs(r["gf"] - 2.0 * want.real).max() < 1e-11
        assert np.abs(r["gq"] - 2.0 * np.abs(want)).max() < 1e-11
        assert np.abs(want.imag).max() > 1e-5 and r["before"] and r["pool_plans"] == 1
        assert r["reads"] > 0 and r["info"]["streaming_fallback"] == 0
        if label == "widened":
            assert not r["after"] and r["sigma_dtype"] == "torch.complex128"
        else:
            assert r["after"] and r["sigma_dtype"] == "torch.float64"
            assert r["real_reads"] == r["reads"]


def _flow_problem():
    from openvqe_amd import fermion
    ham, gens, hf = fermion.synthetic_molecule(6, 2, 31)
    pool = fermion.uccsd_pool_antihermitian(6, 2)
    return ham, pool, hf


def _flow_worker(rank, world, port, chunk_bits, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["OVQE_SHARD_CHUNK_BITS"] = str(chunk_bits)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from openvqe_amd.backend import GRAD_FERMIONIC, GRAD_QUBIT
        from openvqe_amd.partitioned import PartitionedStatevector
        ham, pool, hf = _flow_problem()
        with PartitionedStatevector(12, device=0) as sv:
            sv.set_hamiltonian(ham)
            sv.init_basis(hf)
            real0 = sv.sharded._storage_real()
            sv.apply_exp_pauli_sum(pool[0], 0.21)
            sv.apply_exp_pauli_sum(pool[-1], -0.4)
            real1 = sv.sharded._storage_real()
            gf = sv.pool_gradients(pool, GRAD_FERMIONIC)
            gq = sv.pool_gradients(pool, GRAD_QUBIT)
            real2 = sv.sharded._storage_real()
            plans = sv.sharded.engine.counters["pool_plans"]
            n2 = sv.norm2()
        if rank == 0:
            out.put((gf, gq, (real0, real1, real2), plans, n2))
    finally:
        dist.destroy_process_group()


def test_partitioned_adapt_flow_screens_on_doubles(gpu_lib):
    """``init_basis``, ``apply_exp_pauli_sum`` of two JW generators, ``pool_gradients`` through PartitionedStatevector on two HIP shards:
    float64 shards before and after, the values of the one-device handle"""
    from openvqe_amd.backend import GRAD_FERMIONIC, GRAD_QUBIT, Statevector
    gf, gq, reals, plans, n2 = _spawn(_flow_worker, 2, (11,))
    ham, pool, hf = _flow_problem()
    with Statevector(12) as sv:
        sv.set_hamiltonian(ham)
        sv.init_basis(hf)
        sv.apply_exp_pauli_sum(pool[0], 0.21)
        sv.apply_exp_pauli_sum(pool[-1], -0.4)
        wf = np.asarray(sv.pool_gradients(pool, GRAD_FERMIONIC))
        wq = np.asarray(sv.pool_gradients(pool, GRAD_QUBIT))
    print("max error fermionic %.3e qubit %.3e" % (np.abs(gf - wf).max(), np.abs(gq - wq).max()))
    assert reals == (True, True, True) and plans == 1 and abs(n2 - 1.0) < 1e-12
    assert np.abs(gf - wf).max() < 1e-11 and np.abs(gq - wq).max() < 1e-11
    assert np.abs(wf).max() > 1e-3
