"""bench.py's N > 1 path on one GPU: two processes (torch.distributed over gloo, both ranks on device 0 — RCCL refuses two
ranks on one device) run the replica benchmark; rank 0 must print ONE well-formed JSON line with the contract's keys and
the whole-job aggregate over both ranks."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _strict_json(text):
    def refuse(name):
        raise ValueError(f"non-standard JSON constant {name}")
    return json.loads(text, parse_constant=refuse)


def test_two_process_replica_bench_line(gpu_lib):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, OVQE_BENCH_BACKEND="gloo", OVQE_BENCH_SINGLE_DEVICE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
           "--batch", "2048", "--no-roofline", "--no-cpu", "--no-extra", "--no-sharded"]   # (the sharded block: the next test, at a size the oracle holds)
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    assert len(lines[0]) < 4096      # the driver's parser lost round 4's 22-KB line
    out = _strict_json(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config"):
        assert key in out, key
    assert out["n_gpus"] == 2 and out["steps"] == 3 and out["warmup"] == 1 and out["scaling"] == "weak"
    assert out["unit"] == "evals/s" and out["dtype"] == "f64" and out["vs_baseline"] is None
    assert "workload" in out["config"] and out["config"]["parallelism"].endswith("x2")
    # whole-job aggregate: both ranks' batches over the max-over-ranks time
    assert abs(out["value"] - 2 * 2048 * 3 / (out["ms_per_step"] * 3e-3)) < 1e-6 * out["value"]


def test_two_process_sharded_block_against_oracle(gpu_lib):
    """configs[4] through the plain command `python bench.py --gpus 2` at a size the oracle holds (gloo, both ranks on
    device 0): the parent starts the two ranks itself, and the line must carry the `sharded` block — weak run at n = 16 (one global qubit), strong run at n = 15 — and both energies
    must equal the bit-mask oracle's on the host-recomputed synthetic state."""
    import numpy as np

    import bench
    from openvqe_amd import synth
    from oracle import masks
    # the PLAIN command, no launcher and no WORLD_SIZE: bench.py starts its own two ranks (a fresh child, never exec)
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(OVQE_BENCH_BACKEND="gloo", OVQE_BENCH_SINGLE_DEVICE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--batch", "1024", "--no-roofline", "--no-cpu", "--no-extra", "--sharded-qubits", "15", "--sharded-rotations", "24",
           "--sharded-terms", "80"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    last = r.stdout.strip().splitlines()[-1]                # the JSON line is the LAST line
    assert len(last) < 4096
    out = _strict_json(last)
    assert out["n_gpus"] == 2 and out["config"]["parallelism"].endswith("x2")
    assert out["sharded"]["weak_qubits"] == 16 and out["sharded"]["strong_qubits"] == 15
    assert out["sharded"]["energy_check"] == "no value on record for these sizes"
    sh = json.load(open(os.path.join(ROOT, out["extra"])))["sharded"]     # the legs' detail: bench_extra.json, named by the line
    assert sh["weak"]["energy"] == out["sharded"]["weak_energy"] and sh["strong"]["energy"] == out["sharded"]["strong_energy"]
    assert sh["weak"]["n_qubits"] == 16 and sh["strong"]["n_qubits"] == 15
    for leg in (sh["weak"], sh["strong"]):
        n = leg["n_qubits"]
        xs, zs, phis, hx, hz, hc = bench.sharded_workload(n, 24, 80)
        psi = synth.amplitudes(bench.SHARDED_SEED, np.arange(1 << n, dtype=np.uint64))
        psi = psi / np.linalg.norm(psi)
        for x, z, p in zip(xs, zs, phis):
            psi = masks.rotate(psi, x, z, p)
        want = masks.expectation(psi, hx, hz, hc, 0.0)
        assert abs(leg["energy"] - want) < 1e-11 * np.abs(hc).sum(), (n, leg["energy"], want)
        assert abs(leg["norm2"] - 1.0) < 1e-12
        assert leg["n_gpus"] == 2 and leg["swaps"] >= 1 and leg["exchanged_GiB_per_rank"] > 0
        assert leg["xgmi_link_GBs_exchange"] > 0 and leg["full_shard_reads"] >= 1
        # the per-rank compute seconds of the scaling proxy (ranks on one device take their compute sections in turn)
        assert leg["local_sweeps_s"] > 0 and leg["expectation_local_s"] > 0 and leg["expectation_remote_compute_s"] >= 0
        assert leg["exchange_count"] == leg["swaps"] and leg["projected_with_xgmi"]["rotations_s"] > 0
    assert len(out["sharded"]["weak_compute_s"]) == 3


def test_stalled_rank_ends_the_sharded_leg_with_a_line_and_exit_code_3(gpu_lib):
    """One rank never posts its half of the first exchange (injected): the watchdog over the collective waits
    (openvqe_amd.distributed.DistWatchdog, OVQE_DIST_TIMEOUT_S) makes rank 0 print the line — contract keys and the replica
    figures intact, "sharded": {"error": ...} — and every process leaves with a non-zero exit code within seconds, instead of
    sitting in the wait until the driver's limit."""
    import time
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(OVQE_BENCH_BACKEND="gloo", OVQE_BENCH_SINGLE_DEVICE="1", HSA_ENABLE_IPC_MODE_LEGACY="0",
               OVQE_DIST_TIMEOUT_S="6", OVQE_BENCH_INJECT_STALL_RANK="1")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--batch", "1024", "--no-roofline", "--no-cpu", "--no-extra", "--sharded-qubits", "15", "--sharded-rotations", "24",
           "--sharded-terms", "80"]
    t0 = time.perf_counter()
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert time.perf_counter() - t0 < 300
    assert r.returncode != 0
    last = r.stdout.strip().splitlines()[-1]
    assert len(last) < 4096
    out = _strict_json(last)
    assert out["n_gpus"] == 2 and out["value"] > 0 and out["metric"] == "vqe_energy_evals_per_sec"
    assert "no progress" in out["sharded"]["error"] and "OVQE_DIST_TIMEOUT_S" in out["sharded"]["error"]


def test_failing_sharded_leg_still_prints_the_line(gpu_lib):
    """An exception inside the partitioned block (injected on every rank; a failed collective looks like this) must not cost the line:
    rank 0 prints it with the replica figures and "sharded": {"error": ...}, the processes leave with a non-zero exit code at once"""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(OVQE_BENCH_BACKEND="gloo", OVQE_BENCH_SINGLE_DEVICE="1", HSA_ENABLE_IPC_MODE_LEGACY="0",
               OVQE_BENCH_INJECT_SHARDED_ERROR="1")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--batch", "1024", "--no-roofline", "--no-cpu", "--no-extra", "--sharded-qubits", "15", "--sharded-rotations", "24",
           "--sharded-terms", "80"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode != 0
    last = r.stdout.strip().splitlines()[-1]
    out = _strict_json(last)
    assert out["n_gpus"] == 2 and out["value"] > 0 and "injected failure" in out["sharded"]["error"]


def test_single_gpu_sharded_leg_checks_its_energy_against_the_value_on_record(gpu_lib):
    """`sharded.energy_check`: the 31-qubit energy of configs[4]'s strong leg does not depend on the number of GPUs; the value of the
    one-GPU run is on record (bench.SHARDED_KNOWN) and every run compares with it to 1e-11 |H|_1.  Here: the record mechanism on a
    small register against the bit-mask oracle (the 31-qubit leg itself is part of `bench.py --full`)."""
    import numpy as np

    import bench
    from openvqe_amd import synth
    from oracle import masks
    n, R, T = 18, 24, 80
    xs, zs, phis, hx, hz, hc = bench.sharded_workload(n, R, T)
    psi = synth.amplitudes(bench.SHARDED_SEED, np.arange(1 << n, dtype=np.uint64))
    psi = psi / np.linalg.norm(psi)
    for x, z, p in zip(xs, zs, phis):
        psi = masks.rotate(psi, x, z, p)
    want = masks.expectation(psi, hx, hz, hc, 0.0)
    bench.SHARDED_KNOWN[(n, R, T)] = want
    try:
        leg = bench.sharded_leg(n, 0, 1, 0, R, T)
        assert leg["energy_check"]["ok"] and leg["energy_check"]["abs_diff"] < 1e-11 * np.abs(hc).sum()
        bench.SHARDED_KNOWN[(n, R, T)] = want + 1e-6
        leg = bench.sharded_leg(n, 0, 1, 0, R, T)
        assert not leg["energy_check"]["ok"]
    finally:
        del bench.SHARDED_KNOWN[(n, R, T)]


def test_plain_run_times_the_headline_only_and_dumps_the_last_step(gpu_lib, tmp_path):
    """`bench.py --gpus 1` without --full: the line carries the contract's keys and none of the side legs; --dump-outputs
    writes the B energies of the last timed step, which equal the C oracle's on that step's parameter block (step 3 of
    warm-up 1 + 3 timed steps: block 3 of the seeded draw)"""
    import numpy as np

    import bench
    from oracle import cref
    from openvqe_amd.backend import compile_ucc_program
    B = 512
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", str(B),
           "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    out = _strict_json(r.stdout.strip().splitlines()[-1])
    assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0 and out["dtype"] == "f64"
    assert abs(out["value"] - B * 3 / (out["ms_per_step"] * 3e-3)) < 1e-6 * out["value"]
    for side in ("roofline", "cpu_baseline", "sharded", "side"):
        assert side not in out, side
    e = np.load(os.path.join(str(tmp_path), "energies.npy"))
    assert e.dtype == np.float64 and e.shape == (B,)
    ham, gens, hf = bench.build_workload()
    thetas = np.random.default_rng(140).uniform(-0.1, 0.1, size=(4, B, len(gens)))[3]
    rx, rz, rc, pidx, _ = compile_ucc_program(ham.nbqbits, gens)
    hx, hz, hc = ham.packed()
    want = cref.ucc_energy_batch(ham.nbqbits, hf, rx, rz, rc, pidx, thetas[:16], hx, hz, hc.real.copy(), ham.constant_coeff)
    assert np.abs(e[:16] - want).max() < 1e-10, np.abs(e[:16] - want).max()
