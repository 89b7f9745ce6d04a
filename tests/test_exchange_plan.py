"""The exchange planner of the partitioned register on the CPU, at full size: which index bits each exchange trades for the 64-rotation
benchmark workload at 34 qubits on 8 ranks and 33 qubits on 4 — no engine is touched (a program compiled without a Hamiltonian is
pure bookkeeping).  A k-bit exchange puts S / 2^k on its busiest link (S = one shard) and sends (1 - 2^-k) S in all."""
import numpy as np
import pytest

import bench
from openvqe_amd.distributed import ShardedStatevector, permute_mask


def _plan(n, world, bits=None, rotations=64):
    xs, zs, phis, _, _, _ = bench.sharded_workload(n, rotations, 1000)
    sv = ShardedStatevector(n, engine_factory=lambda *a: None, dry_rank=(world, 0))
    if bits is not None:
        sv.max_exchange_bits = bits
    prog = sv.compile_program(xs, zs, np.ones(len(xs)), np.arange(len(xs)), 0)
    return sv, prog, [int(x) for x in xs]


def _link(prog):
    return sum(2.0 ** -k for k in prog["exchange_bits"])        # in shards: busiest link, summed over the (serial) exchanges


def _sent(prog):
    return sum(1.0 - 2.0 ** -k for k in prog["exchange_bits"])


def _check_plan_is_executable(sv, prog, xs):
    """replay the steps on a permutation: every rotation's physical x mask is local at its step, every exchange trades distinct
    global bits for distinct local bits that the rotations after it (up to the next exchange) do not need, the end is a permutation"""
    n, nl = sv.n, sv.n_local
    perm = list(range(n))
    seen = 0
    for st in prog["steps"]:
        if st[0] == "swap":
            gbits, lbits = st[1], st[2]
            assert len(gbits) == len(lbits) >= 1 and len(set(gbits)) == len(gbits) and len(set(lbits)) == len(lbits)
            assert all(nl <= b < n for b in gbits) and all(0 <= b < nl for b in lbits)
            for gb, lb in zip(gbits, lbits):
                a, b = perm.index(gb), perm.index(lb)
                perm[a], perm[b] = lb, gb
        else:
            for r, xp in zip(st[3], st[1]):
                assert int(xp) == permute_mask(xs[int(r)], perm) and int(xp) >> nl == 0
                seen += 1
    assert seen == len(xs)
    assert perm == prog["perm"] and sorted(perm) == list(range(n))
    assert prog["swaps"] == len(prog["exchange_bits"]) == sum(1 for st in prog["steps"] if st[0] == "swap")
    assert prog["exchange_bits"] == [len(st[1]) for st in prog["steps"] if st[0] == "swap"]


@pytest.mark.parametrize("n,world,one_bit,ratio", [(34, 8, (9, 4.5), 1 / 4), (33, 4, (6, 3.0), 1 / 3)])
def test_multibit_plan_of_the_benchmark_workload(n, world, one_bit, ratio):
    sv1, p1, xs = _plan(n, world, bits=1)
    assert (p1["swaps"], _link(p1)) == one_bit and set(p1["exchange_bits"]) == {1}      # the half-shard plan as it always was
    _check_plan_is_executable(sv1, p1, xs)
    sv, p, _ = _plan(n, world)
    assert sv.max_exchange_bits == sv.g
    _check_plan_is_executable(sv, p, xs)
    print(f"{n} q / {world}: 1-bit {p1['swaps']} exchanges, link {_link(p1)} S, sent {_sent(p1)} S; "
          f"default {p['exchange_bits']}, link {_link(p)} S, sent {_sent(p)} S")
    assert _link(p) <= ratio * _link(p1)
    assert _sent(p) <= _sent(p1)
    assert p["swaps"] <= p1["swaps"]
    assert max(p["exchange_bits"]) > 1


def test_exchange_bits_bound_and_environment(monkeypatch):
    sv, p, xs = _plan(34, 8, bits=2)
    _check_plan_is_executable(sv, p, xs)
    assert max(p["exchange_bits"]) == 2
    assert _link(p) < 4.5
    monkeypatch.setenv("OVQE_EXCHANGE_BITS", "1")
    sv, p, _ = _plan(34, 8)
    assert sv.max_exchange_bits == 1 and p["swaps"] == 9 and set(p["exchange_bits"]) == {1}
    monkeypatch.setenv("OVQE_EXCHANGE_BITS", "7")            # never more than the rank bits
    assert _plan(20, 4)[0].max_exchange_bits == 2


def test_plan_is_the_same_on_every_rank_and_world_2_keeps_the_half_shard_plan():
    xs, zs, _, _, _, _ = bench.sharded_workload(16, 64, 10)
    plans = []
    for rank in range(8):
        sv = ShardedStatevector(16, engine_factory=lambda *a: None, dry_rank=(8, rank))
        prog = sv.compile_program(xs, zs, np.ones(64), np.arange(64), 0)
        plans.append([(st[1], st[2]) for st in prog["steps"] if st[0] == "swap"])
    assert all(p == plans[0] for p in plans) and len(plans[0]) >= 1
    # one rank bit: nothing to combine — the plan is the Belady half-shard plan, exchange for exchange
    sv2, p2, xs2 = _plan(20, 2)
    sv1, p1, _ = _plan(20, 2, bits=1)
    assert sv2.max_exchange_bits == 1
    assert [(st[1], st[2]) for st in p2["steps"] if st[0] == "swap"] == [(st[1], st[2]) for st in p1["steps"] if st[0] == "swap"]
    _check_plan_is_executable(sv2, p2, xs2)
    # ... as recorded from the half-shard planner before multi-bit exchanges existed (bench workload, 20 qubits, 2 ranks)
    assert [(st[1], st[2]) for st in p2["steps"] if st[0] == "swap"] == [((19,), (1,)), ((19,), (12,)), ((19,), (11,)), ((19,), (8,))]


def test_a_rotation_wider_than_a_shard_is_refused():
    sv = ShardedStatevector(8, engine_factory=lambda *a: None, dry_rank=(8, 0))
    with pytest.raises(ValueError, match="more qubits than fit in one shard"):
        sv.compile_program([0b11111100], [0], [1.0], [0], 0)
    # n - |x| = g: exactly the rank bits are left over, and the plan exists
    prog = sv.compile_program([0b11111000], [0], [1.0], [0], 0)
    assert prog["swaps"] >= 1 and sum(prog["exchange_bits"]) == 3
