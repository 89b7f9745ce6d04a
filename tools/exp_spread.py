"""Energy spread S = ||(H - omega) psi||^2 with energies and exact gradients of a batch in one launch: ovqe_spread_gradient_batch
(Statevector.spread_gradient_batch) of H2O/STO-3G UCCSD — 14 qubits, K = 140 — or LiH at B = 1024 and 4096, in variance mode and with
omega given, beside ovqe_energy_gradient_batch on the same handle in the same process, the two calls alternating.
  python tools/exp_spread.py [--mol H2O|LiH] [--reps N] [--out DIR]
Times: the HIP events of the calls' own info entries (theta to the device + the launch), medians after a warm-up.  Per configuration:
both times, their ratio, and the geometry each call chose.  One JSON line per configuration (and DIR/spread_<mol>.json)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    import numpy as np
    from openvqe_amd import chem, fermion
    from openvqe_amd.backend import Statevector
    name, reps, out_dir = _arg("--mol", "H2O"), _arg("--reps", 11), _arg("--out", "")
    mol = chem.molecule(name)
    mol.rhf()
    ham, gens, hf = mol.jw_hamiltonian(), fermion.uccsd_generators(mol.nao, mol.n_elec // 2), mol.hf_init()
    K, n = len(gens), ham.nbqbits
    rng = np.random.default_rng(2)
    med = lambda v: float(np.median(v))   # noqa: E731
    rows = []
    with Statevector(n) as sv:
        sv.set_hamiltonian(ham)
        sv.set_ucc_program(gens, hf)
        for B in (1024, 4096):
            thetas = rng.uniform(-0.2, 0.2, (B, K))
            e_ref = sv.energy_gradient_batch(thetas)[0]
            for mode, omega in (("variance", None), ("omega given", e_ref + 0.05)):
                for _ in range(2):   # warm-up: buffers, code objects
                    sv.spread_gradient_batch(thetas, omega, 0.3, 1.0)
                    sv.energy_gradient_batch(thetas)
                spread, plain = [], []
                for _ in range(reps):
                    c, g, e, s = sv.spread_gradient_batch(thetas, omega, 0.3, 1.0)
                    spread.append(sv.spread_info())
                    e0, g0 = sv.energy_gradient_batch(thetas)
                    plain.append(sv.gradient_batch_info())
                info = spread[-1]
                t_spread, t_plain = med([i["launch_us"] for i in spread]), med([i["launch_us"] for i in plain])
                row = {"mol": name, "qubits": n, "K": K, "B": B, "mode": mode, "info": info, "plain_info": plain[-1],
                       "spread_launch_us": t_spread, "plain_launch_us": t_plain, "ratio": t_spread / t_plain,
                       "per_row_kernel_us": t_spread / B, "plain_per_row_kernel_us": t_plain / B,
                       "copy_back_us": med([i["copy_back_us"] for i in spread]),
                       "energies_equal_bits": bool(np.array_equal(e.view(np.int64), e0.view(np.int64))),
                       "spread_min_max": [float(s.min()), float(s.max())]}
                rows.append(row)
                print(json.dumps(row), flush=True)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, f"spread_{name}.json"), "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
