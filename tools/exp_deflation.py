"""Deflated energies and gradients of a batch in one launch: ovqe_deflated_gradient_batch (Statevector.deflated_gradient_batch) of
H2O/STO-3G UCCSD — 14 qubits, K = 140 — or LiH at B = 1024 and 4096 with J = 0, 1 and 4 real vectors and J = 4 complex vectors, beside
ovqe_energy_gradient_batch on the same handle in the same process, the two calls alternating.
  python tools/exp_deflation.py [--mol H2O|LiH] [--reps N] [--out DIR]
Times: the HIP events of the calls' own info entries (theta to the device + the launch), medians after a warm-up.  Per configuration:
the ratio to the undeflated call (J = 0: expected near 1) and the cost per real row, (deflated - undeflated of the same B) / rows.  One
JSON line per configuration (and DIR/deflation_<mol>.json)."""
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
        for J, complex_vectors in ((0, False), (1, False), (4, False), (4, True)):
            sv.deflation_truncate(0)
            for j in range(J):
                if complex_vectors:        # a dense random vector: weight on and off the support, Re and Im rows
                    v = rng.normal(size=1 << n) + 1j * rng.normal(size=1 << n)
                    sv.set_state(v / np.linalg.norm(v))
                else:                      # an ansatz state: real on the support
                    sv.prepare_state(rng.uniform(-0.2, 0.2, K))
                sv.deflation_push(1.0 + j)
            for B in (1024, 4096):
                thetas = rng.uniform(-0.2, 0.2, (B, K))
                for _ in range(2):   # warm-up: buffers, code objects, the gather
                    sv.deflated_gradient_batch(thetas)
                    sv.energy_gradient_batch(thetas)
                defl, plain = [], []
                for _ in range(reps):
                    c, g, e, o = sv.deflated_gradient_batch(thetas)
                    defl.append(sv.deflation_info())
                    e0, g0 = sv.energy_gradient_batch(thetas)
                    plain.append(sv.gradient_batch_info())
                info = defl[-1]
                t_defl, t_plain = med([i["launch_us"] for i in defl]), med([i["launch_us"] for i in plain])
                row = {"mol": name, "qubits": n, "K": K, "B": B, "J": J, "complex": complex_vectors, "real_rows": info["rows"], "info": info,
                       "plain_info": plain[-1], "deflated_launch_us": t_defl, "plain_launch_us": t_plain, "ratio": t_defl / t_plain,
                       "per_gradient_kernel_us": t_defl / B, "plain_per_gradient_kernel_us": t_plain / B,
                       "us_per_real_row_and_batch": (t_defl - t_plain) / info["rows"] if info["rows"] else None,
                       "ns_per_real_row_and_gradient": 1e3 * (t_defl - t_plain) / info["rows"] / B if info["rows"] else None,
                       "copy_back_us": med([i["copy_back_us"] for i in defl]),
                       "energies_equal_bits": bool(np.array_equal(e.view(np.int64), e0.view(np.int64))),
                       "max_gradient_difference_at_J0": float(np.abs(g - g0).max()) if J == 0 else None}
                rows.append(row)
                print(json.dumps(row), flush=True)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, f"deflation_{name}.json"), "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
