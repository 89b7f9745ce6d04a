"""Fubini-Study metric of a UCCSD state on the compact-support path: ovqe_metric_tensor (Statevector.metric_tensor) of H2O/STO-3G
UCCSD — 14 qubits, K = 140 — against its yardstick, ovqe_energy_batch with B = 2 K evaluations on the same handle: the same number of
circuit executions on the same kernel family, plus an <H> that the tangent kernel does not do.  The tangent stage is allowed up to
twice the batch's time (it writes one support-sized vector per parameter to HBM and has no row schedule).
  python tools/exp_metric.py [--mol H2O|LiH] [--reps N] [--out DIR]
Times: HIP events of ovqe_metric_info (tangents, Gram, finish), wall clock around the synchronous calls, and the HIP events of
ovqe_last_batch_ms for the same batch resident on the device (ovqe_energy_batch_device); medians after a warm-up.  One JSON line
(and DIR/metric_<mol>.json)."""
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
    name, reps, out_dir = _arg("--mol", "H2O"), _arg("--reps", 21), _arg("--out", "")
    mol = chem.molecule(name)
    mol.rhf()
    ham, gens, hf = mol.jw_hamiltonian(), fermion.uccsd_generators(mol.nao, mol.n_elec // 2), mol.hf_init()
    K = len(gens)
    rng = np.random.default_rng(2)
    theta = rng.uniform(-0.2, 0.2, K)
    batch = rng.uniform(-0.2, 0.2, (2 * K, K))
    med = lambda v: float(np.median(v))   # noqa: E731
    with Statevector(ham.nbqbits) as sv:
        sv.set_hamiltonian(ham)
        sv.set_ucc_program(gens, hf)
        for _ in range(3):   # warm-up: tables, buffers, code objects
            g = sv.metric_tensor(theta)
            sv.energy_batch(batch)
        wall, infos = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            g = sv.metric_tensor(theta)
            wall.append(time.perf_counter() - t0)
            infos.append(sv.metric_info())
        bwall, bdev = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            sv.energy_batch(batch)
            bwall.append(time.perf_counter() - t0)
        forms = sorted(sv.sparse_forms())
        # the same batch resident on the device: that call is bracketed by HIP events (a batch of this size from the host travels through
        # the mapped buffer and is not)
        import torch
        th = torch.tensor(batch, dtype=torch.float64, device="cuda")
        en = torch.empty(2 * K, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        for _ in range(reps + 3):
            sv.energy_batch_device(2 * K, th.data_ptr(), en.data_ptr())
            bdev.append(sv.last_batch_ms())
        bdev = bdev[3:]
        forms_dev = sorted(sv.sparse_forms())
    info = infos[-1]
    res = {"mol": name, "qubits": ham.nbqbits, "K": K, "metric_info": info,
           "tangents_us": med([i["tangents_us"] for i in infos]), "gram_us": med([i["gram_us"] for i in infos]),
           "finish_us": med([i["finish_us"] for i in infos]), "metric_wall_us": 1e6 * med(wall),
           "batch_B": 2 * K, "batch_forms": forms, "batch_wall_us": 1e6 * med(bwall),
           "batch_device_forms": forms_dev, "batch_device_us": 1e3 * med(bdev),
           "symmetric": bool(np.array_equal(g, g.T)), "smallest_eigenvalue": float(np.linalg.eigvalsh(g)[0]),
           "largest_diagonal": float(np.max(np.diag(g)))}
    res["tangents_over_batch_device"] = res["tangents_us"] / res["batch_device_us"] if res["batch_device_us"] > 0 else None
    res["tangents_over_batch_wall"] = res["tangents_us"] / res["batch_wall_us"]
    print(json.dumps(res), flush=True)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, f"metric_{name}.json"), "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
