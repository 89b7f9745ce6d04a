"""Exact energy Hessian of a UCCSD state on the compact-support path: ovqe_energy_hessian (Statevector.energy_hessian) of H2O/STO-3G
UCCSD — 14 qubits, K = 140 — or LiH, against the only route the library offered before it: central differences of the exact gradient,
2 K ``energy_gradient`` calls in the same process.
  python tools/exp_hessian.py [--mol H2O|LiH] [--reps N] [--step H] [--out DIR] [--once]
Times: HIP events of ovqe_hessian_info (the launch, the copy back), wall clock around the synchronous calls; medians after a warm-up.
Also the largest deviation of the central-difference Hessian from the exact one.  ``--once``: three calls and nothing else (the run to
put under a kernel trace).  One JSON line (and DIR/hessian_<mol>.json)."""
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
    name, reps, step, out_dir = _arg("--mol", "H2O"), _arg("--reps", 21), _arg("--step", 1e-5), _arg("--out", "")
    mol = chem.molecule(name)
    mol.rhf()
    ham, gens, hf = mol.jw_hamiltonian(), fermion.uccsd_generators(mol.nao, mol.n_elec // 2), mol.hf_init()
    K = len(gens)
    theta = np.random.default_rng(2).uniform(-0.2, 0.2, K)
    med = lambda v: float(np.median(v))   # noqa: E731
    with Statevector(ham.nbqbits) as sv:
        sv.set_hamiltonian(ham)
        sv.set_ucc_program(gens, hf)
        for _ in range(3):   # warm-up: plan, buffers, code objects
            e, g, hs = sv.energy_hessian(theta)
            sv.energy_gradient(theta)
        if "--once" in sys.argv:
            print(json.dumps({"mol": name, "K": K, "hessian_info": sv.hessian_info()}), flush=True)
            return
        wall, infos = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            e, g, hs = sv.energy_hessian(theta)
            wall.append(time.perf_counter() - t0)
            infos.append(sv.hessian_info())
        gwall = []
        for _ in range(reps):
            t0 = time.perf_counter()
            sv.energy_gradient(theta)
            gwall.append(time.perf_counter() - t0)
        cd = np.zeros((K, K))
        t0 = time.perf_counter()
        for k in range(K):
            tp, tm = theta.copy(), theta.copy()
            tp[k] += step
            tm[k] -= step
            cd[k] = (sv.energy_gradient(tp)[1] - sv.energy_gradient(tm)[1]) / (2 * step)
        cd_wall = time.perf_counter() - t0
        forms = sorted(sv.sparse_forms())
    info = infos[-1]
    cd = 0.5 * (cd + cd.T)
    res = {"mol": name, "qubits": ham.nbqbits, "K": K, "hessian_info": info,
           "launch_us": med([i["phase0_us"] for i in infos]), "copy_back_us": med([i["phase1_us"] for i in infos]),
           "hessian_wall_us": 1e6 * med(wall), "gradient_wall_us": 1e6 * med(gwall), "gradient_forms": forms,
           "central_difference_calls": 2 * K, "central_difference_step": step, "central_difference_wall_us": 1e6 * cd_wall,
           "central_difference_max_deviation": float(np.abs(cd - hs).max()), "largest_entry": float(np.abs(hs).max()),
           "asymmetry": info["asymmetry"], "lowest_eigenvalue": float(np.linalg.eigvalsh(hs)[0]),
           "central_difference_over_hessian_wall": 1e6 * cd_wall / (1e6 * med(wall))}
    print(json.dumps(res), flush=True)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, f"hessian_{name}.json"), "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
