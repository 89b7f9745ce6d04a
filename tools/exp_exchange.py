#!/usr/bin/env python3
"""Shard exchanges of the partitioned register, measured on ONE GPU (profiles/r7_exchange/README.md holds the numbers).

  python tools/exp_exchange.py dry [--qubits 34] [--world 8] [--tree DIR]
      a dry rank 0 of `world` (one rank of the job alone: it packs, "receives" its own pieces and unpacks) runs the 64-rotation
      benchmark workload: seconds in exchanges (pack + stand-in copy + unpack, device synchronised on both sides), seconds in local
      sweeps, bytes sent, bytes on the busiest link, and the eight-GPU projection local sweeps + copies + busiest-link bytes / 153 GB/s.
      OVQE_EXCHANGE_BITS=1 gives the half-shard plan.  --tree imports the package from another checkout (before / after runs: the
      script uses nothing but ShardedStatevector and its stats; a checkout without "link_bytes" has every exchange on one link).
  python tools/exp_exchange.py kernels [--local-qubits 28]
      pack and unpack of one block by the engine's kernels (only where the engine offers `pack`), HIP events on the engine's stream,
      2 warm-up + 5 timed runs each: exchanged bits low / middle / top, k = 1..3, 16-byte amplitudes, 8-byte amplitudes (float64 shard)
      and real parts of a complex shard; bytes moved per second as a fraction of the 6.29 TB/s copy ceiling of the MI355X; for k = 1
      the torch strided copies (`.contiguous()` / `.copy_()`) of the same half beside them.
One JSON line per result on stdout."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XGMI_LINK_GBS = 153.0
COPY_CEILING_GBS = 6290.0


def dry(args):
    import bench
    import torch
    from openvqe_amd.distributed import ShardedStatevector
    n, world = args.qubits, args.world
    g = world.bit_length() - 1
    xs, zs, phis, _, _, _ = bench.sharded_workload(n, 64, 1000)
    sv = ShardedStatevector(n, device=0, dry_rank=(world, 0))
    sv.randomize(bench.SHARDED_SEED)
    if args.real:
        sv.engine.set_real(True)
        sv.real = True
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sv.apply_pauli_rotations(xs, zs, phis)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    st = sv.stats
    shard = (8 if args.real else 16) * 2 ** (n - g)
    link = st.get("link_bytes", st["bytes_sent"])
    out = {"what": "dry rank", "qubits": n, "world": world, "amplitude_bytes": 8 if args.real else 16, "shard_GiB": shard / 2 ** 30,
           "max_exchange_bits": getattr(sv, "max_exchange_bits", 1), "exchanges": st["swaps"], "exchange_bits": st.get("exchange_bits", st["swaps"]),
           "pieces": st["pieces"], "bytes_sent_in_shards": st["bytes_sent"] / shard, "busiest_link_in_shards": link / shard,
           "exchange_copies_s": st["swap_s"], "local_sweeps_s": st["local_sweeps_s"], "rotations_wall_s": wall,
           # pack, stand-in copy and unpack each read and write what is sent (blocks sent from where they lie skip the pack)
           "copies_TBs_if_all_three_ran": 6.0 * st["bytes_sent"] / st["swap_s"] / 1e12 if st["swap_s"] > 0 else None,
           "projected_8gpu_rotations_s": st["local_sweeps_s"] + st["swap_s"] + link / (XGMI_LINK_GBS * 1e9),
           "projection_assumes": "busiest-link bytes at 153 GB/s, all links of an exchange concurrently; RCCL rates unmeasured"}
    print(json.dumps(out), flush=True)


def kernels(args):
    import torch
    from openvqe_amd.distributed import HipShardEngine
    nl = args.local_qubits
    eng = HipShardEngine(nl, 3, 0, 0)
    if not hasattr(eng, "pack"):
        print(json.dumps({"what": "kernels", "skipped": "the engine of this checkout offers no pack / unpack"}), flush=True)
        return
    eng.randomize(1, 1.0)

    def timed(fn):
        for _ in range(2):
            fn()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
        ev[0].record(eng.stream)
        for i in range(5):
            fn()
            ev[i + 1].record(eng.stream)
        torch.cuda.synchronize()
        return min(ev[i].elapsed_time(ev[i + 1]) for i in range(5)) * 1e-3

    for storage in ("complex", "real_parts_only", "float64"):
        if storage == "float64":
            eng.set_real(True)
        rpo = storage == "real_parts_only"
        ebytes = 16 if storage == "complex" else 8
        for k in (1, 2, 3):
            mid = nl // 2
            for where, mask in (("low", (1 << k) - 1), ("low+1", ((1 << k) - 1) << 1), ("middle", ((1 << k) - 1) << mid),
                                ("scattered", sum(1 << b for b in (1, mid, nl - 2)[:k])), ("top", ((1 << k) - 1) << (nl - k))):
                bsize = 1 << (nl - k)
                buf = torch.empty(bsize, dtype=torch.float64 if ebytes == 8 else torch.complex128, device=eng.device)
                block = (1 << k) - 1
                t_pack = timed(lambda: eng.pack(mask, block, 0, bsize, buf, rpo))
                t_unpack = timed(lambda: eng.unpack(mask, block, 0, bsize, buf, rpo))
                # bytes through HBM: the stream once, the shard side once (real parts only: whole 16-byte amplitudes on the shard side)
                moved = bsize * (ebytes + (16 if rpo else ebytes))
                row = {"what": "kernel", "storage": storage, "k": k, "bits": where, "mask": mask, "block_MiB": bsize * ebytes / 2 ** 20,
                       "pack_ms": 1e3 * t_pack, "unpack_ms": 1e3 * t_unpack, "pack_TBs": moved / t_pack / 1e12, "unpack_TBs": moved / t_unpack / 1e12,
                       "pack_frac_of_copy_ceiling": moved / t_pack / 1e9 / COPY_CEILING_GBS,
                       "unpack_frac_of_copy_ceiling": moved / t_unpack / 1e9 / COPY_CEILING_GBS}
                if k == 1:     # the torch copies a half-shard exchange used before: the strided half of the same bit
                    lbit = mask.bit_length() - 1
                    half = eng.tensor.view(1 << (nl - 1 - lbit), 2, 1 << lbit)[:, 1, :]
                    if rpo:
                        t_tp = timed(lambda: torch.view_as_real(half)[..., 0].contiguous())

                        def back():
                            dst = torch.view_as_real(half)
                            dst[..., 0].copy_(buf.view(half.shape))
                            dst[..., 1].zero_()
                        t_tu = timed(back)
                    else:
                        t_tp = timed(lambda: half.contiguous())
                        t_tu = timed(lambda: half.copy_(buf.view(half.shape)))
                    row.update({"torch_pack_ms": 1e3 * t_tp, "torch_unpack_ms": 1e3 * t_tu, "torch_pack_TBs": moved / t_tp / 1e12,
                                "torch_unpack_TBs": moved / t_tu / 1e12})
                print(json.dumps(row), flush=True)
                del buf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["dry", "kernels"])
    ap.add_argument("--qubits", type=int, default=34)
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--real", action="store_true", help="float64 shards (the workload keeps a real state real)")
    ap.add_argument("--local-qubits", type=int, default=28)
    ap.add_argument("--tree", default=ROOT)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    dry(args) if args.mode == "dry" else kernels(args)


if __name__ == "__main__":
    main()
