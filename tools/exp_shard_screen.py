#!/usr/bin/env python3
"""The ADAPT gradient screen on the partitioned register, measured with two REAL ranks on one GPU (gloo, host-staged partner reads; the
timed compute sections take the device in turn through a lock file).  profiles/shard_screen/README.md holds the numbers.

  python tools/exp_shard_screen.py [--qubits 28] [--ops 1246] [--terms 200] [--reps 3] [--state adapt|dense] [--tree DIR]

The pool is synthetic in the shape of the H2O UCCSD pool: ``--ops`` anti-Hermitian Jordan-Wigner excitations (one in twelve a single:
2 strings; the others doubles: 8 strings on one x mask), orbitals drawn over the whole register.  The Hamiltonian is a seeded
real-symmetric sum (tools/exp_real_apply.py).  ``adapt``: a basis state under a few odd-Y rotations (real, on a few tiles — what an
ADAPT iteration screens); ``dense``: a seeded dense real vector.  ``--tree`` imports the package from another checkout (before / after
runs: the script uses nothing but ShardedStatevector.pool_gradients, its stats and the engine's counters; a checkout whose stats have no
"screen_s" reports the wall time of the call alone).  One JSON line per (rank, repeat)."""
import argparse
import json
import os
import socket
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def synthetic_pool(n, ops, seed=5):
    import numpy as np
    rng = np.random.default_rng(seed)
    pool = []

    def chain(lo, hi):
        return sum(1 << b for b in range(lo + 1, hi))

    for k in range(ops):
        if k % 12 == 0:      # single excitation i/2 (X_p Z.. Y_q - Y_p Z.. X_q)
            p, q = sorted(int(b) for b in rng.choice(n, 2, replace=False))
            x = (1 << p) | (1 << q)
            zc = chain(p, q)
            pool.append(([x, x], [zc | (1 << q), zc | (1 << p)], [0.5j, -0.5j]))
            continue
        p, q, r, s = sorted(int(b) for b in rng.choice(n, 4, replace=False))
        x = (1 << p) | (1 << q) | (1 << r) | (1 << s)
        zc = chain(p, q) | chain(r, s)
        xs, zs, cs = [], [], []
        for pat in range(16):          # the 8 patterns with an odd number of Y
            if bin(pat).count("1") & 1:
                y = sum(1 << b for i, b in enumerate((p, q, r, s)) if (pat >> i) & 1)
                xs.append(x)
                zs.append(zc | y)
                cs.append((0.125j if bin(pat).count("1") == 1 else -0.125j) * (1 if pat in (1, 2, 7, 11) else -1))
        pool.append((xs, zs, cs))
    return pool


def rank_main(rank, world, port, args, lock):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    sys.path.insert(0, os.path.abspath(args.tree))
    import numpy as np
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        sys.path.insert(1, ROOT)
        from tools.exp_real_apply import hamiltonian
        from openvqe_amd.distributed import ShardedStatevector
        n = args.qubits
        hx, hz, hc = hamiltonian(n, args.terms)
        pool = synthetic_pool(n, args.ops)
        sv = ShardedStatevector(n, device=0)
        sv.compute_lock = lock
        rng = np.random.default_rng(3)
        if args.state == "adapt":
            rots = []
            for _ in range(6):
                bits = [int(b) for b in rng.choice(n - 1, 4, replace=False)]     # (local x masks: no exchange, the permutation stays)
                x = sum(1 << b for b in bits)
                rots.append((x, (1 << bits[0]) | (int(rng.integers(0, 1 << n)) & ~x), float(rng.uniform(0.2, 1.0))))
            sv._choose_storage(True)
            sv.init_basis(int(rng.integers(0, 1 << n)))
            sv.apply_pauli_rotations([r[0] for r in rots], [r[1] for r in rots], [r[2] for r in rots])
        else:
            sv._choose_storage(True)
            sv.engine.randomize(11, 1.0)
            sv.real = True
        start_real = sv._storage_real()
        ham = (hx, hz, hc, 0.0)
        for rep in range(-1, args.reps):       # (repeat -1: plans, LDS opt-in, buffers)
            if rep >= 0 and start_real and not sv._storage_real() and hasattr(sv.engine, "set_real"):
                sv.engine.set_real(True)       # a checkout that widens for the screen starts every repeat from the float64 shard
                sv._tmp = sv._chunk_bufs = None
            before = dict(sv.stats)
            cnt = dict(sv.engine.counters)
            torch.cuda.synchronize()
            dist.barrier()
            t0 = time.perf_counter()
            g = sv.pool_gradients(ham, pool, "fermionic")
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            if rep < 0:
                continue
            d = {k: sv.stats[k] - before.get(k, 0) for k in sv.stats if isinstance(sv.stats[k], (int, float))}
            row = {"rank": rank, "repeat": rep, "qubits": n, "local_qubits": sv.n_local, "chunk_bits": sv._chunk_bits(), "ops": len(pool),
                   "state": args.state, "storage_before": "float64" if start_real else "complex128",
                   "storage_after": "float64" if sv._storage_real() else "complex128",
                   "pool_gradients_wall_s": round(wall, 4), "screen_s": round(d["screen_s"], 4) if "screen_s" in d else None,
                   "sigma_apply_s": round(d["apply_s"], 4), "partner_read_wait_s": round(d["shard_read_s"], 4),
                   "link_bytes": d["bytes_sent"], "chunk_reads": d["chunk_reads"],
                   "contraction_passes": sv.engine.counters["contraction_passes"] - cnt["contraction_passes"],
                   "contraction_bytes_by_construction": sv.engine.counters["contraction_bytes"] - cnt["contraction_bytes"],
                   "pool_plans": sv.engine.counters.get("pool_plans"), "g_abs_sum": float(np.abs(g).sum())}
            print(json.dumps(row), flush=True)
    finally:
        dist.destroy_process_group()


def main():
    import torch.multiprocessing as mp
    ap = argparse.ArgumentParser()
    ap.add_argument("--qubits", type=int, default=28)
    ap.add_argument("--ops", type=int, default=1246)
    ap.add_argument("--terms", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--world", type=int, default=2)
    ap.add_argument("--state", choices=["adapt", "dense"], default="adapt")
    ap.add_argument("--tree", default=ROOT)
    args = ap.parse_args()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    with tempfile.TemporaryDirectory() as tmp:
        ctx = mp.get_context("spawn")
        procs = [ctx.Process(target=rank_main, args=(r, args.world, port, args, os.path.join(tmp, "device.lock"))) for r in range(args.world)]
        for p in procs:
            p.start()
        for p in procs:
            p.join()
        sys.exit(max(abs(p.exitcode or 0) for p in procs))


if __name__ == "__main__":
    main()
