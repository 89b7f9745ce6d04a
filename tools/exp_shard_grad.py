#!/usr/bin/env python3
"""The adjoint gradient on the partitioned register, measured on ONE GPU (profiles/shard_gradient/README.md holds the numbers).

  python tools/exp_shard_grad.py kernel [--local-qubits 28]
      one shard, the 64-rotation list of bench.sharded_workload on its local qubits, random psi and lambda: the backward pass
      (ovqe_adjoint_rotations) in its tiled forms ("adjoint_tile_bits" 11 and 12: k_tile_adjoint) and in the streaming-only form (0:
      k_adjoint_pairs per same-x run), and the forward sweep (ovqe_apply_pauli_rotations: k_tile_sweep) on the same list as the
      yardstick.  1 warm-up + 3 timed calls each, HIP events on the engine's stream, the fastest kept; passes, ms, bytes per second
      at 64 B per amplitude and pass (forward: 32 B).
  python tools/exp_shard_grad.py e2e [--qubits 34] [--world 8] [--tree DIR]
      a dry rank 0 of `world` (one rank of the job alone; exchanges and partner reads move its own data: every kernel and every copy
      of the real job, no link): the benchmark workload as a compiled program with K = 64 parameters — seconds for one
      program_energy and for one program_energy_gradient (1 warm-up + 2 timed each, the faster kept), and the ratio of the gradient to
      K + 1 energies (what forward differences cost).  --tree imports the package from another checkout: a checkout without
      program_energy_gradient reports the energy alone (the parent's side of the comparison).
One JSON line per result on stdout."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XGMI_LINK_GBS = 153.0


def kernel(args):
    import numpy as np
    import torch
    import bench
    from openvqe_amd.distributed import HipShardEngine
    nl = args.local_qubits
    xs, zs, phis, _, _, _ = bench.sharded_workload(nl, 64, 8)
    xs, zs, phis = np.array(xs, np.uint64), np.array(zs, np.uint64), np.array(phis, np.float64)
    runs = 1 + int(np.count_nonzero(xs[1:] != xs[:-1]))
    eng = HipShardEngine(nl, 0, 0, 0)
    eng.randomize(1, 1.0)
    lam = torch.view_as_complex(torch.randn(1 << nl, 2, dtype=torch.float64, device=eng.device))
    namps = float(1 << nl)

    def timed(fn):
        fn()
        best = None
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(eng.stream)
            fn()
            e1.record(eng.stream)
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1)
            best = ms if best is None else min(best, ms)
        return best

    fwd_ms = timed(lambda: eng.sv.apply_pauli_rotations(xs, zs, phis))
    fwd_passes, fwd_bytes = eng.sv.last_passes()
    print(json.dumps({"what": "forward sweep", "local_qubits": nl, "rotations": 64, "same_x_runs": runs, "passes": fwd_passes, "ms": fwd_ms,
                      "TBs": fwd_bytes / fwd_ms / 1e9}), flush=True)
    for bits in (0, 11, 12):
        eng.sv.set_option("adjoint_tile_bits", bits)
        ms = timed(lambda: eng.sv.adjoint_rotations(lam.data_ptr(), xs, zs, phis))
        passes, nbytes = eng.sv.last_passes()
        assert nbytes == 64 * namps * passes
        print(json.dumps({"what": "backward pass", "form": "streaming" if bits == 0 else "tiles of 2^%d" % bits, "local_qubits": nl,
                          "passes": passes, "ms": ms, "TBs": nbytes / ms / 1e9, "ms_over_forward": ms / fwd_ms}), flush=True)


def e2e(args):
    import numpy as np
    import torch
    import bench
    from openvqe_amd.distributed import ShardedStatevector
    n, world = args.qubits, args.world
    xs, zs, phis, hx, hz, hc = bench.sharded_workload(n, 64, 1000)
    K = len(xs)
    sv = ShardedStatevector(n, device=0, dry_rank=(world, 0))
    prog = sv.compile_program(xs, zs, np.ones(K), np.arange(K), 0, hamiltonian=(hx, hz, hc, 0.0))
    theta = np.asarray(phis, np.float64)

    def timed(fn):
        fn()
        best = None
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        return best

    def snapshot():
        return dict(sv.stats), dict(sv.engine.counters)

    t_e = timed(lambda: sv.program_energy(prog, theta))
    out = {"what": "dry rank", "qubits": n, "world": world, "K": K, "real_program": bool(prog["real"]), "exchanges": prog["swaps"],
           "exchange_bits": prog["exchange_bits"], "program_energy_s": t_e, "forward_differences_s": (K + 1) * t_e}
    if hasattr(sv, "program_energy_gradient"):
        t_g = timed(lambda: sv.program_energy_gradient(prog, theta))
        s0, c0 = snapshot()
        sv.program_energy_gradient(prog, theta)
        s1, c1 = snapshot()
        d = {k: s1[k] - s0[k] for k in ("swap_s", "local_sweeps_s", "adjoint_sweeps_s", "apply_s", "shard_read_s", "link_bytes", "bytes_sent")}
        out.update({"program_energy_gradient_s": t_g, "gradient_over_energy": t_g / t_e, "gradient_over_forward_differences": t_g / ((K + 1) * t_e),
                    "adjoint_passes": c1["adjoint_passes"] - c0["adjoint_passes"], "adjoint_bytes": c1["adjoint_bytes"] - c0["adjoint_bytes"],
                    "seconds_by_phase": {k: d[k] for k in ("swap_s", "local_sweeps_s", "adjoint_sweeps_s", "apply_s", "shard_read_s")},
                    "busiest_link_GB": d["link_bytes"] / 1e9,
                    # one rank's compute and copies as measured + its busiest-link bytes at the xGMI rate (exchanges only: the partner
                    # reads of H psi overlap their contractions)
                    "projected_8gpu_gradient_s": t_g + d["link_bytes"] / (XGMI_LINK_GBS * 1e9),
                    "projection_assumes": "busiest-link bytes at 153 GB/s, all links of an exchange concurrently; RCCL rates unmeasured"})
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernel", "e2e"])
    ap.add_argument("--local-qubits", type=int, default=28)
    ap.add_argument("--qubits", type=int, default=34)
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--tree", default=ROOT)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    kernel(args) if args.mode == "kernel" else e2e(args)


if __name__ == "__main__":
    main()
