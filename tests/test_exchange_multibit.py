"""k-bit shard exchanges (ShardedStatevector._swap_bits: k global index bits for k local ones in one all-to-all among 2^k ranks) over
gloo at world size 4 and 8, shard arithmetic by the bit-mask oracle engine of tests/test_distributed.py, which offers no pack /
unpack: the torch indexing fall-back moves the blocks.  The same workers run on HIP shards in tests/test_gpu_exchange.py."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import masks
from tests.test_distributed import OracleShardEngine, _free_port


def exchange_lists(n, world, seed):
    """a general rotation list and an odd-Y one (a real state stays real), both with X/Y on two and on all rank bits at once, and a
    Hamiltonian with x anywhere"""
    rng = np.random.default_rng(seed)
    g = world.bit_length() - 1
    R, T = 26, 24

    def xmask(maxw):
        return sum(1 << int(b) for b in rng.choice(n, int(rng.integers(1, maxw + 1)), replace=False))

    xs = [xmask(min(4, n - g - 1)) for _ in range(R)]
    zs = [int(v) for v in rng.integers(0, 1 << n, R)]
    xs[2] = 0b11 << (n - 2)
    xs[9] = ((1 << g) - 1) << (n - g)
    xs[15] = (1 << (n - 1)) | (1 << (n - g)) | 1
    xs[21] = (0b11 << (n - g)) | 0b110
    phis = rng.uniform(-1, 1, R)
    rx, rz = [], []
    for r in range(R):
        bits = [int(b) for b in rng.choice(n, int(rng.integers(2, 5)), replace=False)]
        if r in (3, 12):
            bits = [n - 1, n - 2, 0, 3]
        if r in (7, 18):
            bits = list(range(n - g, n)) + [1]
        x = sum(1 << b for b in bits)
        z = (1 << bits[-1]) | (int(rng.integers(0, 1 << n)) & ~x)      # one Y, Z elsewhere
        rx.append(x)
        rz.append(z)
    rphis = rng.uniform(-1, 1, R)
    hx = [xmask(3) if rng.random() < 0.8 else 0 for _ in range(T)]
    hz = [int(v) for v in rng.integers(0, 1 << n, T)]
    hc = rng.normal(size=T)
    hf = int(rng.integers(0, 1 << n))
    return (xs, zs, phis), (rx, rz, rphis), (hx, hz, hc), hf


def exchange_worker(rank, world, port, n, seed, out, engine="oracle"):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["OVQE_SHARD_CHUNK_BITS"] = str(max(2, n - (world.bit_length() - 1) - 2))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from openvqe_amd.distributed import ShardedStatevector
        (xs, zs, phis), (rx, rz, rphis), (hx, hz, hc), hf = exchange_lists(n, world, seed)

        def make(bits=None):
            sv = (ShardedStatevector(n, device=0) if engine == "hip" else
                  ShardedStatevector(n, engine_factory=lambda nl, ng, r: OracleShardEngine(nl, ng, r)))
            if bits is not None:
                sv.max_exchange_bits = bits
            return sv

        def run(sv, x, z, p, real_program=False):
            sv._choose_storage(real_program)
            sv.init_basis(hf)
            sv.apply_pauli_rotations(x, z, p)
            st = dict(sv.stats)                       # (before <H>: its partner reads count into bytes_sent too)
            stored = sv._storage_real()
            e = sv.expectation(hx, hz, hc, 0.25)
            n2 = sv.norm2()
            return {"e": e, "n2": n2, "stats": st, "stored": stored, "dtype": str(sv.engine.tensor.dtype), "full": sv.gather_state()}

        res = {}
        sv = make()
        res["max_bits"] = sv.max_exchange_bits
        res["default"] = run(sv, xs, zs, phis)
        res["one_bit"] = run(make(1), xs, zs, phis)
        # the same list as a compiled program: planned once, same exchanges
        sv = make()
        prog = sv.compile_program(xs, zs, phis, np.zeros(len(xs), np.int64), hf, hamiltonian=(hx, hz, hc, 0.25))
        sv.run_program(prog, [1.0])
        st = dict(sv.stats)
        res["program"] = {"e": sv._expectation_planned(prog["ham"]), "stats": st, "bits": list(prog["exchange_bits"]),
                          "swaps": prog["swaps"], "full": sv.gather_state()}
        # odd-Y list: float64 shards where the engine has them / real parts on the wire / complex wire
        for variant in ("stored", True, False):
            sv = make()
            sv.real_storage = variant == "stored"
            sv.real_transfers = variant is not False
            res[("real", variant)] = run(sv, rx, rz, rphis, real_program=True)
        sv = make()
        res["real_bits"] = list(sv.compile_program(rx, rz, rphis, np.zeros(len(rx), np.int64), hf)["exchange_bits"])
        if rank == 0:
            out.put(res)
    finally:
        dist.destroy_process_group()


def launch(world, n, seed, engine="oracle", timeout=300):
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=exchange_worker, args=(r, world, port, n, seed, out, engine)) for r in range(world)]
    for p in procs:
        p.start()
    res = out.get(timeout=timeout)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    return res


def check_exchange_results(res, world, n, seed, hip=False):
    g = world.bit_length() - 1
    (xs, zs, phis), (rx, rz, rphis), (hx, hz, hc), hf = exchange_lists(n, world, seed)

    def oracle(x, z, p):
        psi = np.zeros(1 << n, complex)
        psi[hf] = 1
        for a, b, c in zip(x, z, p):
            psi = masks.rotate(psi, int(a), int(b), c)
        return psi, masks.expectation(psi, hx, hz, hc, 0.25)

    psi, want = oracle(xs, zs, phis)
    shard = 16 << (n - g)                                    # bytes of one complex shard

    def predicted(bits, ebytes=16):
        s = (shard // 16) * ebytes
        return sum(s >> k for k in bits), sum(s - (s >> k) for k in bits)

    assert res["max_bits"] == g
    for key in ("default", "one_bit", "program"):
        r = res[key]
        assert np.abs(np.asarray(r["full"]) - psi).max() < 1e-12, key
        assert abs(r["e"] - want) < 1e-11, key
    assert abs(res["default"]["n2"] - 1.0) < 1e-12
    assert np.abs(np.asarray(res["default"]["full"]) - np.asarray(res["one_bit"]["full"])).max() < 1e-12
    st, st1, stp, bits = res["default"]["stats"], res["one_bit"]["stats"], res["program"]["stats"], res["program"]["bits"]
    print(f"world {world}, n {n}: exchanges of {bits} bits; 1-bit plan {st1['swaps']} exchanges; "
          f"link bytes {st['link_bytes']} vs {st1['link_bytes']}, sent {st['bytes_sent']} vs {st1['bytes_sent']}")
    assert st["exchange_bits"] > st["swaps"] >= 1            # a multi-bit exchange really happened
    assert max(bits) == g                                    # ... on all rank bits at once (the list has X/Y on all of them)
    assert st["swaps"] == stp["swaps"] == res["program"]["swaps"] == len(bits) and st["exchange_bits"] == stp["exchange_bits"] == sum(bits)
    assert (st["link_bytes"], st["bytes_sent"]) == predicted(bits) == (stp["link_bytes"], stp["bytes_sent"])
    assert st["real_exchanges"] == 0
    assert st1["exchange_bits"] == st1["swaps"] and st1["link_bytes"] == st1["bytes_sent"] == st1["swaps"] * (shard // 2)
    assert st["link_bytes"] < st1["link_bytes"]
    # the odd-Y list: real parts on the wire are half the bytes of the same list forced complex
    rpsi, rwant = oracle(rx, rz, rphis)
    assert np.abs(rpsi.imag).max() < 1e-15
    for variant in ("stored", True, False):
        r = res[("real", variant)]
        assert np.abs(np.asarray(r["full"]) - rpsi).max() < 1e-12, variant
        assert abs(r["e"] - rwant) < (1e-10 * np.abs(hc).sum() if r["stored"] else 1e-11), variant
    s1, s0, ss = res[("real", True)]["stats"], res[("real", False)]["stats"], res[("real", "stored")]["stats"]
    rbits = res["real_bits"]
    assert max(rbits) == g and s1["swaps"] == s0["swaps"] == ss["swaps"] == len(rbits)
    assert s1["real_exchanges"] == s1["swaps"] and s0["real_exchanges"] == 0
    assert (s0["link_bytes"], s0["bytes_sent"]) == predicted(rbits, 16)
    assert (s1["link_bytes"], s1["bytes_sent"]) == predicted(rbits, 8) == (ss["link_bytes"], ss["bytes_sent"])
    assert 2 * s1["bytes_sent"] == s0["bytes_sent"] and 2 * s1["link_bytes"] == s0["link_bytes"]
    # float64 shards stay float64 through a k-bit exchange (engines with real storage: the HIP engine)
    assert res[("real", "stored")]["stored"] == hip
    assert res[("real", "stored")]["dtype"] == ("torch.float64" if hip else "torch.complex128")
    assert not res[("real", True)]["stored"] and not res[("real", False)]["stored"]


@pytest.mark.parametrize("world,n", [(4, 10), (8, 11), (8, 13), (4, 12)])
def test_multibit_exchange_matches_single_process_oracle(world, n):
    seed = 700 + 10 * world + n
    check_exchange_results(launch(world, n, seed), world, n, seed)


class RecordingEngine(OracleShardEngine):
    """an engine that offers pack / unpack: does them with numpy and notes every call"""

    def __init__(self, n_local, n_global, rank):
        super().__init__(n_local, n_global, rank)
        self.calls = []

    def _index(self, mask, block, first, count):
        j = np.arange(first, first + count, dtype=np.int64)
        out, i, src = np.zeros_like(j), 0, 0
        for bit in range(self.n_local):
            if (mask >> bit) & 1:
                out |= ((block >> i) & 1) << bit
                i += 1
            else:
                out |= ((j >> src) & 1) << bit
                src += 1
        return out

    def pack(self, mask, block, first, count, dst, real_parts_only=False):
        self.calls.append(("pack", mask, block, first, count, bool(real_parts_only)))
        v = self.tensor.numpy()[self._index(mask, block, first, count)]
        dst.numpy()[:] = v.real if real_parts_only else v

    def unpack(self, mask, block, first, count, src, real_parts_only=False):
        self.calls.append(("unpack", mask, block, first, count, bool(real_parts_only)))
        self.tensor.numpy()[self._index(mask, block, first, count)] = src.numpy()


@pytest.mark.parametrize("rank", [0, 5])
@pytest.mark.parametrize("real", [False, True])
def test_an_engine_with_pack_and_unpack_gets_every_block_and_piece(rank, real):
    """dry rank of an 8-rank register: a 3-bit exchange on scattered local bits and a 1-bit one.  Every block but the rank's own is
    packed and unpacked, in ranges that tile it exactly once, pack before unpack; a dry rank receives what it sent, so the shard is
    unchanged; the byte counts are those of the real rank: 7/8 of the shard sent, 1/8 on the busiest link"""
    from openvqe_amd.distributed import ShardedStatevector
    n, nl = 12, 9
    sv = ShardedStatevector(n, engine_factory=RecordingEngine, dry_rank=(8, rank))
    eng = sv.engine
    rng = np.random.default_rng(5)
    eng.tensor.copy_(torch.from_numpy(rng.normal(size=1 << nl) + (0 if real else 1j) * rng.normal(size=1 << nl)))
    sv.real = real
    before = eng.tensor.clone()
    sv._swap_bits([nl + 2, nl, nl + 1], [6, 0, 3])
    ebytes = 8 if real else 16
    assert sv.stats["swaps"] == 1 and sv.stats["exchange_bits"] == 3 and sv.stats["real_exchanges"] == int(real)
    assert sv.stats["bytes_sent"] == 7 * (ebytes << nl) // 8 and sv.stats["link_bytes"] == (ebytes << nl) // 8
    assert torch.equal(eng.tensor, before)
    # the pairs in ascending order of the local bit: (0, nl), (3, nl + 1), (6, nl + 2) — this rank's own block spells its coordinate
    own = ((rank >> 0) & 1) | (((rank >> 1) & 1) << 1) | (((rank >> 2) & 1) << 2)
    mask = 0b1001001
    bsize = 1 << (nl - 3)
    for what in ("pack", "unpack"):
        calls = [c for c in eng.calls if c[0] == what]
        assert all(c[1] == mask and c[5] == real for c in calls)
        assert sorted(set(c[2] for c in calls)) == [b for b in range(8) if b != own]
        for b in set(c[2] for c in calls):
            ranges = sorted((c[3], c[4]) for c in calls if c[2] == b)
            assert len(ranges) == sv.EXCHANGE_PIECES == sv.stats["pieces"]
            assert ranges[0][0] == 0 and all(a[0] + a[1] == c[0] for a, c in zip(ranges, ranges[1:])) and sum(ranges[-1]) == bsize
    for b in range(8):
        if b != own:
            order = [c[0] for c in eng.calls if c[2] == b and c[3] == 0]
            assert order == ["pack", "unpack"]
    # the logical qubits on each pair traded places
    assert [sv.perm[q] for q in (0, 3, 6, nl, nl + 1, nl + 2)] == [nl, nl + 1, nl + 2, 0, 3, 6]
    # k = 1 on the same engine: the half-shard exchange, one partner
    eng.calls.clear()
    sv._swap_bits([nl + 1], [4])
    assert sv.stats["swaps"] == 2 and sv.stats["exchange_bits"] == 4
    assert sv.stats["link_bytes"] == (ebytes << nl) // 8 + (ebytes << nl) // 2
    assert {c[2] for c in eng.calls} == {1 - ((rank >> 1) & 1)} and {c[1] for c in eng.calls} == {1 << 4}
    assert sum(c[4] for c in eng.calls if c[0] == "pack") == 1 << (nl - 1) == sum(c[4] for c in eng.calls if c[0] == "unpack")
    assert torch.equal(eng.tensor, before)


def test_top_bit_blocks_are_sent_from_where_they_lie():
    """blocks that are contiguous in the shard (the top local bits, complex wire) need no pack: unpack calls only"""
    from openvqe_amd.distributed import ShardedStatevector
    sv = ShardedStatevector(10, engine_factory=RecordingEngine, dry_rank=(4, 2))
    sv.engine.tensor.copy_(torch.arange(256, dtype=torch.float64).to(torch.complex128))
    before = sv.engine.tensor.clone()
    sv._swap_bits([9, 8], [7, 6])
    assert {c[0] for c in sv.engine.calls} == {"unpack"} and torch.equal(sv.engine.tensor, before)
    assert sv.stats["bytes_sent"] == 3 * 16 * 64 and sv.stats["link_bytes"] == 16 * 64
    with pytest.raises(ValueError, match="distinct"):
        sv._swap_bits([9, 9], [1, 2])
    with pytest.raises(ValueError, match="distinct"):
        sv._swap_bits([9], [8])
