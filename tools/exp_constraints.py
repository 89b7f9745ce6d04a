"""Observables beside the Hamiltonian in one launch: ovqe_constrained_gradient_batch (Statevector.constrained_gradient_batch) of
H2O/STO-3G UCCSD — 14 qubits, K = 140 — or LiH at B = 4096, beside ovqe_energy_gradient_batch and ovqe_deflated_gradient_batch on the
same handle in the same process, the calls alternating within every repetition:
  plain            energy_gradient_batch
  deflated_J0      deflated_gradient_batch with no vector
  M0               the constrained call with no observable
  M2_zero          S^2 and N held, weights zero (pass one only: the expectation values of a batch)
  M2_weighted      quad weights on both (pass one and pass two)
  M2_weighted_J4   ... and four real vectors
  python tools/exp_constraints.py [--mol H2O|LiH] [--B N] [--reps N] [--out DIR]
Times: the HIP events of the calls' own info entries (theta to the device + the launch), medians after a warm-up, and the ratios to the
plain gradient of the same run.  One JSON line per configuration (and DIR/constraints_<mol>.json)."""
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
    name, B, reps, out_dir = _arg("--mol", "H2O"), _arg("--B", 4096), _arg("--reps", 11), _arg("--out", "")
    mol = chem.molecule(name)
    mol.rhf()
    ham, gens, hf = mol.jw_hamiltonian(), fermion.uccsd_generators(mol.nao, mol.n_elec // 2), mol.hf_init()
    K, n = len(gens), ham.nbqbits
    rng = np.random.default_rng(2)
    thetas = rng.uniform(-0.2, 0.2, (B, K))
    s2, number = fermion.spin_squared(n), fermion.number_operator(n)
    quad, target = np.array([1.5, 0.75]), np.array([0.0, float(mol.n_elec)])
    med = lambda v: float(np.median(v))   # noqa: E731
    with Statevector(n) as sv:
        sv.set_hamiltonian(ham)
        sv.set_ucc_program(gens, hf)

        def vectors(J):
            sv.deflation_truncate(0)
            for j in range(J):
                sv.prepare_state(rng.uniform(-0.2, 0.2, K))
                sv.deflation_push(1.0 + j)

        def observables(M):
            sv.observable_truncate(0)
            for op in (s2, number)[:M]:
                sv.observable_push(op)

        def constrained(M, weighted, J):
            def call():
                if sv.observable_count() != M:
                    observables(M)
                if sv.deflation_count() != J:
                    vectors(J)
                out = sv.constrained_gradient_batch(thetas, quad=quad[:M] if weighted else None, target=target[:M] if weighted else None)
                return sv.constraint_info(), out
            return call

        def plain():
            out = sv.energy_gradient_batch(thetas)
            return sv.gradient_batch_info(), out

        def deflated():
            if sv.deflation_count():
                vectors(0)
            out = sv.deflated_gradient_batch(thetas)
            return sv.deflation_info(), out

        configs = [("plain", plain), ("deflated_J0", deflated), ("M0", constrained(0, False, 0)), ("M2_zero", constrained(2, False, 0)),
                   ("M2_weighted", constrained(2, True, 0)), ("M2_weighted_J4", constrained(2, True, 4))]
        infos = {key: [] for key, _ in configs}
        last = {}
        for rep in range(reps + 2):          # two warm-up rounds: buffers, code objects, the gather, the restriction
            for key, call in configs:
                for _ in range(2):           # (the second call of a configuration: the cached rows and entries serve)
                    info, out = call()
                if rep >= 2:
                    infos[key].append(info)
                last[key] = out
    t_plain = med([i["launch_us"] for i in infos["plain"]])
    rows = []
    for key, _ in configs:
        info = infos[key][-1]
        t = med([i["launch_us"] for i in infos[key]])
        row = {"mol": name, "qubits": n, "K": K, "B": B, "config": key, "launch_us": t, "ratio_to_plain": t / t_plain,
               "min_launch_us": float(min(i["launch_us"] for i in infos[key])), "copy_back_us": med([i["copy_back_us"] for i in infos[key]]),
               "per_gradient_kernel_us": t / B, "info": info}
        if key in ("deflated_J0", "M0"):
            row["energies_equal_plain_bits"] = bool(np.array_equal(last[key][2].view(np.int64), last["plain"][0].view(np.int64)))
        if key.startswith("M2"):
            row["mean_values"] = [float(x) for x in last[key][3].mean(axis=0)]
        rows.append(row)
        print(json.dumps(row), flush=True)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, f"constraints_{name}.json"), "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
