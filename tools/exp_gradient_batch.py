"""Exact gradients of a batch of parameter vectors in one launch: ovqe_energy_gradient_batch (Statevector.energy_gradient_batch) of
H2O/STO-3G UCCSD — 14 qubits, K = 140 — or LiH at B = 1, 8, 64, 256, 1024, 4096, against, in the same process,
  (a) B sequential ``energy_gradient`` calls (the only exact route before it: one workgroup per call), and
  (b) the forward-difference gradient through ``energy_batch`` with B (K + 1) rows (B = 1024 and up: in chunks of 64 gradients).
  python tools/exp_gradient_batch.py [--mol H2O|LiH] [--reps N] [--waves 0|1|2|4|8] [--out DIR]
Times: the HIP events of ovqe_gradient_batch_info (theta to the device + the launch; the copy back) and the wall clock around the
synchronous calls; medians after a warm-up.  ``--waves``: option "grad_batch_waves" (0: the planner's choice).  One JSON line per batch
size (and DIR/gradient_batch_<mol>[_w<waves>].json)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    import numpy as np
    from openvqe_amd import chem, fermion
    from openvqe_amd.backend import Statevector
    name, reps, waves, out_dir = _arg("--mol", "H2O"), _arg("--reps", 11), _arg("--waves", 0), _arg("--out", "")
    mol = chem.molecule(name)
    mol.rhf()
    ham, gens, hf = mol.jw_hamiltonian(), fermion.uccsd_generators(mol.nao, mol.n_elec // 2), mol.hf_init()
    K = len(gens)
    rng = np.random.default_rng(2)
    med = lambda v: float(np.median(v))   # noqa: E731
    eps = float(np.sqrt(np.finfo(float).eps))
    rows = []
    with Statevector(ham.nbqbits) as sv:
        sv.set_option("grad_batch_waves", waves)
        sv.set_hamiltonian(ham)
        sv.set_ucc_program(gens, hf)
        for B in (1, 8, 64, 256, 1024, 4096):
            thetas = rng.uniform(-0.2, 0.2, (B, K))
            for _ in range(2):   # warm-up: buffers, code objects
                e, g = sv.energy_gradient_batch(thetas)
            wall, infos = [], []
            for _ in range(reps):
                t0 = time.perf_counter()
                e, g = sv.energy_gradient_batch(thetas)
                wall.append(time.perf_counter() - t0)
                infos.append(sv.gradient_batch_info())
            # (a) the same rows one call at a time (at most 256 of them are timed: the cost per call does not depend on B)
            nseq = min(B, 256)
            sv.energy_gradient(thetas[0])
            t0 = time.perf_counter()
            seq = [sv.energy_gradient(thetas[b]) for b in range(nseq)]
            seq_wall = (time.perf_counter() - t0) / nseq
            dev = max(float(np.abs(g[b] - seq[b][1]).max()) for b in range(nseq))
            # (b) forward differences through the batched energies, 64 gradients per call at the most
            nfd = min(B, 64)
            pts = np.repeat(thetas[:nfd], K + 1, axis=0).reshape(nfd, K + 1, K)
            pts[:, 1:, :] += eps * np.eye(K)[None]
            pts = pts.reshape(nfd * (K + 1), K)
            sv.energy_batch(pts)
            fd_wall = []
            for _ in range(max(3, reps // 3)):
                t0 = time.perf_counter()
                vals = sv.energy_batch(pts).reshape(nfd, K + 1)
                fd_wall.append((time.perf_counter() - t0) / nfd)
            fd = (vals[:, 1:] - vals[:, :1]) / eps
            info = infos[-1]
            row = {"mol": name, "qubits": ham.nbqbits, "K": K, "B": B, "info": info,
                   "launch_us": med([i["launch_us"] for i in infos]), "copy_back_us": med([i["copy_back_us"] for i in infos]),
                   "wall_us": 1e6 * med(wall), "per_gradient_kernel_us": med([i["launch_us"] for i in infos]) / B,
                   "per_gradient_wall_us": 1e6 * med(wall) / B, "sequential_per_gradient_wall_us": 1e6 * seq_wall,
                   "forward_difference_per_gradient_wall_us": 1e6 * med(fd_wall),
                   "sequential_over_batch": 1e6 * seq_wall / (1e6 * med(wall) / B),
                   "forward_difference_over_batch": 1e6 * med(fd_wall) / (1e6 * med(wall) / B),
                   "max_deviation_from_sequential": dev, "max_deviation_of_forward_differences": float(np.abs(fd - g[:nfd]).max()),
                   "single_forms": sorted(sv.sparse_forms())}
            rows.append(row)
            print(json.dumps(row), flush=True)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, f"gradient_batch_{name}{'_w%d' % waves if waves else ''}.json"), "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
