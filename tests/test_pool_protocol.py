"""CPU tests of the planned ADAPT screen's HOST protocol (ShardedStatevector.pool_gradients with an engine that offers ``plan_pool``):
world sizes 2, 4 and 8 over gloo, the shard arithmetic by the bit-mask oracle engine of tests/test_distributed.py extended by the
``plan_pool`` protocol in numpy — plan cache keyed by (permutation, chunk bits, pool), pool_local while the first chunks travel,
one pool_remote per (partner, chunk), one pool_finish, the all-reduce — against the dense single-process formulas."""
import os

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import masks
from tests.test_distributed import OracleShardEngine, _free_port


class PlannedOracleEngine(OracleShardEngine):
    """the engine protocol of the planned screen: masks in the physical bit space of the whole register, CSR offsets per operator"""

    def __init__(self, n_local, n_global, rank):
        super().__init__(n_local, n_global, rank)
        self.counters = {"pool_plans": 0}
        self.calls = {"local": 0, "remote": 0, "finish": 0, "freed": 0}
        self._pools = {}

    def plan_pool(self, offsets, xs, zs, coeffs, chunk_bits):
        self.counters["pool_plans"] += 1
        pid = max(self._pools, default=-1) + 1
        terms = [(int(xs[t]), int(zs[t]), complex(coeffs[t]), k) for k in range(len(offsets) - 1) for t in range(offsets[k], offsets[k + 1])]
        self._pools[pid] = {"terms": terms, "m": int(chunk_bits), "acc": np.zeros(len(offsets) - 1, complex)}
        return pid

    def free_pool(self, pid):
        self._pools.pop(pid)
        self.calls["freed"] += 1

    def pool_partners(self, pid):
        return [(d, 1) for d in sorted({x >> self.n_local for x, _, _, _ in self._pools[pid]["terms"]} - {0})]

    def pool_info(self, pid):
        return {"operators": len(self._pools[pid]["acc"])}

    def _contract(self, P, m, d, chunk, ket, bra):
        b, k = bra.numpy(), ket.numpy()
        for x, z, c, op in P["terms"]:
            if x >> self.n_local != d:
                continue
            i, sign, ph = self._chunk_form(m, d, chunk, x, z)
            P["acc"][op] += c * ph * np.vdot(b[i], sign * k)

    def pool_local(self, pid, bra):
        self.calls["local"] += 1
        self._contract(self._pools[pid], self.n_local, 0, 0, self.tensor, bra)

    def pool_remote(self, pid, d, chunk, ket, bra):
        self.calls["remote"] += 1
        assert ket.numel() == 1 << self._pools[pid]["m"]
        self._contract(self._pools[pid], self._pools[pid]["m"], d, chunk, ket, bra)

    def pool_finish(self, pid):
        self.calls["finish"] += 1
        out = self._pools[pid]["acc"].copy()
        self._pools[pid]["acc"][:] = 0
        return out


def _protocol_worker(rank, world, port, n, seed, out, planned, chunk_bits):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    if chunk_bits is not None:
        os.environ["OVQE_SHARD_CHUNK_BITS"] = str(chunk_bits)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from openvqe_amd.distributed import ShardedStatevector
        from tests.pool_cases import edge_pool
        rng = np.random.default_rng(seed)
        g = world.bit_length() - 1

        def xmask(maxw):
            return sum(1 << int(b) for b in rng.choice(n, int(rng.integers(1, maxw + 1)), replace=False))

        R, T = 10, 20
        xs = [xmask(max(1, n - g - 1)) & ((1 << (n - g)) - 1) or 1 for _ in range(R)]     # local x masks: the identity permutation stays
        zs = [int(v) for v in rng.integers(0, 1 << n, R)]
        phis = rng.uniform(-1, 1, R)
        hx = [xmask(n) if rng.random() < 0.85 else 0 for _ in range(T)]
        hz = [int(v) for v in rng.integers(0, 1 << n, T)]
        hc = rng.normal(size=T)
        pool = edge_pool(rng, n, n - g, big=False)
        hf = int(rng.integers(0, 1 << n))
        cls = PlannedOracleEngine if planned else OracleShardEngine
        sv = ShardedStatevector(n, engine_factory=lambda nl, ng, r: cls(nl, ng, r))
        sv.init_basis(hf)
        sv.apply_pauli_rotations(xs, zs, phis)
        assert sv.perm == list(range(n))
        ham = (hx, hz, hc, 0.3)
        gf = sv.pool_gradients(ham, pool, "fermionic")
        gq = sv.pool_gradients(ham, pool, "qubit")
        plans_after_two = sv.stats["pool_plans"]
        calls_after_two = dict(getattr(sv.engine, "calls", {}))
        # a rotation with x on the top (rank) qubit: a half-shard exchange changes the permutation -> the pool is planned again
        sv.apply_pauli_rotations([1 << (n - 1)], [3], [0.37])
        perm_changed = sv.perm != list(range(n))
        gf2 = sv.pool_gradients(ham, pool, "fermionic")
        plans_after_three = sv.stats["pool_plans"]
        for k in range(6):        # other pools: the cache keeps the last few plans and frees the evicted ones
            sv.pool_gradients(ham, [([k + 1], [0], [1.0])], "qubit")
        if rank == 0:
            out.put((gf, gq, gf2, plans_after_two, plans_after_three, perm_changed, calls_after_two,
                     dict(getattr(sv.engine, "counters", {})), dict(getattr(sv.engine, "calls", {})), len(sv.__dict__.get("_pool_plans", {})),
                     dict(sv.stats), (xs, zs, phis, hx, hz, hc, pool, hf)))
    finally:
        dist.destroy_process_group()


def _dense_gradients(n, hf, rots, ham, pool):
    psi = np.zeros(1 << n, complex)
    psi[hf] = 1
    for x, z, p in rots:
        psi = masks.rotate(psi, int(x), int(z), p)
    hx, hz, hc = ham
    sigma = 0.3 * psi
    for x, z, c in zip(hx, hz, hc):
        sigma = sigma + c * masks.pauli_apply(psi, int(x), int(z))
    return np.array([sum((c * np.vdot(sigma, masks.pauli_apply(psi, int(x), int(z))) for x, z, c in zip(*op)), 0j) for op in pool])


def _run(world, n, chunk_bits, planned):
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_protocol_worker, args=(r, world, port, n, 1000 + n, out, planned, chunk_bits)) for r in range(world)]
    for p in procs:
        p.start()
    res = out.get(timeout=300)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    return res


@pytest.mark.parametrize("world,n,chunk_bits", [(2, 6, 2), (4, 7, None), (8, 9, 4)])
def test_planned_screen_protocol_matches_dense_formulas(world, n, chunk_bits):
    gf, gq, gf2, plans2, plans3, perm_changed, calls2, counters, calls, kept, stats, (xs, zs, phis, hx, hz, hc, pool, hf) = \
        _run(world, n, chunk_bits, True)
    rots = list(zip(xs, zs, phis))
    want = _dense_gradients(n, hf, rots, (hx, hz, hc), pool)
    assert np.abs(gf - 2.0 * want.real).max() < 1e-11
    assert np.abs(gq - 2.0 * np.abs(want)).max() < 1e-11
    want2 = _dense_gradients(n, hf, rots + [(1 << (n - 1), 3, 0.37)], (hx, hz, hc), pool)
    assert np.abs(gf2 - 2.0 * want2.real).max() < 1e-11
    # two consecutive screens of one pool make exactly one plan; a screen under another permutation makes a second one
    assert plans2 == 1 and perm_changed and plans3 == 2
    g = world.bit_length() - 1
    m = chunk_bits if chunk_bits is not None else max(1, n - g - 2)
    partners = len({(int(x) >> (n - g)) for op in pool for x in op[0]} - {0})
    assert calls2 == {"local": 2, "remote": 2 * partners * (1 << (n - g - m)), "finish": 2, "freed": 0}
    # six more pools: the last few plans are kept, the evicted ones freed
    assert counters["pool_plans"] == stats["pool_plans"] == 8 and kept == 4 and calls["freed"] == 4
    assert stats["screen_s"] > 0.0 and stats["full_shard_reads"] >= 2


def test_engine_without_plan_pool_keeps_the_unplanned_path():
    gf, gq, gf2, plans2, plans3, perm_changed, calls2, counters, calls, kept, stats, (xs, zs, phis, hx, hz, hc, pool, hf) = \
        _run(2, 6, 2, False)
    want = _dense_gradients(6, hf, list(zip(xs, zs, phis)), (hx, hz, hc), pool)
    assert np.abs(gf - 2.0 * want.real).max() < 1e-11 and np.abs(gq - 2.0 * np.abs(want)).max() < 1e-11
    assert plans2 == plans3 == 0 and kept == 0 and stats["screen_s"] == 0.0 and stats["pool_plans"] == 0
