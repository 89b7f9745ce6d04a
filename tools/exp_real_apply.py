"""sigma = H psi on float64 against complex128 shards: per-rank seconds and bytes per sigma of a seeded real-symmetric Pauli sum, two
REAL ranks on one GPU (gloo, host-staged partner reads; the compute sections take the device in turn through a lock file, so the
seconds are each rank's own kernels).  Usage: python tools/exp_real_apply.py [--qubits 30] [--terms 1000] [--reps 2]
One JSON line per (rank, storage)."""
import argparse
import json
import os
import socket
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def hamiltonian(n, terms, seed=7):
    """strings with at most four X / Y (an even number of Y) and Z elsewhere, real coefficients: the shape of a molecular sum"""
    import numpy as np
    rng = np.random.default_rng(seed)
    xs, zs = [], []
    for t in range(terms):
        bits = [int(b) for b in rng.choice(n, int(rng.choice([0, 2, 4])), replace=False)]
        x = sum(1 << b for b in bits)
        y = sum(1 << b for b in bits[:int(rng.choice([0, 2])) if bits else 0])
        xs.append(x)
        zs.append(y | (int(rng.integers(0, 1 << n)) & ~x))
    return np.array(xs, np.uint64), np.array(zs, np.uint64), rng.normal(size=terms)


def rank_main(rank, world, port, args, lock):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from openvqe_amd.distributed import ShardedStatevector
        xs, zs, cs = hamiltonian(args.qubits, args.terms)
        sv = ShardedStatevector(args.qubits, device=0)
        sv.compute_lock = lock
        size = 1 << sv.n_local
        m = sv._chunk_bits()
        for real in (True, False):
            sv.engine.set_real(real, discard=True)
            sv._tmp = sv._chunk_bufs = None
            sv.real = real
            sv.engine.randomize(11, 1.0)
            plan = sv.plan_hamiltonian(xs, zs, cs)
            sigma = sv.engine.new_buffer(size)
            sv._apply_planned(plan, sigma, 0.0)                        # (plans, LDS opt-in, buffers)
            partners = sv.engine.sum_partners(plan["apply"])
            local_passes, local_bytes = sv.engine.sv.last_passes() if not partners else (None, None)
            for key in ("apply_s", "shard_read_s", "bytes_sent"):
                sv.stats[key] = 0
            for _ in range(args.reps):
                sv._apply_planned(plan, sigma, 0.0)
            passes = sum(p for _, p in partners)
            per_amp = 24 if real else 48                                # ket read, sigma read and written
            print(json.dumps({"rank": rank, "storage": "float64" if real else "complex128", "qubits": args.qubits, "local_qubits": sv.n_local,
                              "terms": args.terms, "chunk_bits": m, "sigma_kernel_s": round(sv.stats["apply_s"] / args.reps, 4),
                              "partner_read_wait_s": round(sv.stats["shard_read_s"] / args.reps, 4),
                              "link_bytes_per_sigma": sv.stats["bytes_sent"] // args.reps,
                              "cross_passes_per_chunk": passes, "cross_pass_bytes_per_sigma": passes * per_amp * size,
                              "sigma_norm2_local": float(torch.linalg.vector_norm(sigma).item()) ** 2}), flush=True)
            sv.free_plan(plan)
            del sigma
    finally:
        dist.destroy_process_group()


def main():
    import torch.multiprocessing as mp
    ap = argparse.ArgumentParser()
    ap.add_argument("--qubits", type=int, default=30)
    ap.add_argument("--terms", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--world", type=int, default=2)
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
