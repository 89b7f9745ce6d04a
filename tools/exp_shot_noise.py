"""Shot-noise energies of H2O/STO-3G UCCSD (14 qubits, 1086 Pauli terms): ovqe_energy_sampled (Statevector.energy_sampled) against the
same estimator done on the host from Statevector.get_state() — per measurement group the basis change on the 2^14 amplitudes with
numpy, numpy.cumsum, numpy.searchsorted of the same uniforms, the term signs of every outcome — in the same process on the same state.
  python tools/exp_shot_noise.py [--out DIR] [--reps N] [--host-reps N] [--shots 1024,65536]
Times: wall clock around synchronous calls, median after a warm-up; the split of energy_sampled by phase from the HIP events of
ovqe_measure_info (summed over the groups).  One JSON line per shot count (and DIR/shot_noise_<shots>.json)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def host_estimate(psi, n, xs, zs, cs, const, plan, n_shots, seed):
    """the estimator of include/ovqe_sv.h on the host: -> (energy, std_error)"""
    import numpy as np
    from openvqe_amd import synth
    group, xb, yb = plan
    h = np.array([[1, 1], [1, -1]], complex) / np.sqrt(2)
    hs = h @ np.diag([1, -1j])
    e = const + float(sum(cs[t] for t in range(len(xs)) if group[t] < 0))
    var = 0.0
    for g in range(len(xb)):
        phi = psi.reshape((2,) * n)
        for b in range(n):
            m = h if (int(xb[g]) >> b) & 1 else hs if (int(yb[g]) >> b) & 1 else None
            if m is not None:
                phi = np.moveaxis(np.tensordot(m, phi, axes=([1], [n - 1 - b])), 0, n - 1 - b)
        phi = phi.reshape(-1)
        C = np.cumsum(phi.real ** 2 + phi.imag ** 2)
        idx = np.minimum(np.searchsorted(C, synth.shot_uniforms(seed, g, 0, n_shots) * C[-1], side="right"), C.size - 1).astype(np.uint64)
        v = np.zeros(n_shots)
        for t in np.nonzero(group == g)[0]:
            w = idx & np.uint64(int(xs[t]) | int(zs[t]))
            for s in (32, 16, 8, 4, 2, 1):
                w ^= w >> np.uint64(s)
            v += cs[t] * (1.0 - 2.0 * (w & np.uint64(1)).astype(np.float64))
        e += v.mean()
        var += v.var(ddof=1)
    return e, float(np.sqrt(var / n_shots))


def main():
    import numpy as np
    from openvqe_amd import chem, fermion
    from openvqe_amd.backend import Statevector
    from openvqe_amd.operators import pack_terms
    out_dir = _arg("--out", "")
    reps, host_reps = _arg("--reps", 21), _arg("--host-reps", 3)
    shot_counts = [int(s) for s in _arg("--shots", "1024,65536").split(",")]
    mol = chem.molecule("H2O")
    mol.rhf()
    ham, gens, hf = mol.jw_hamiltonian(), fermion.uccsd_generators(mol.nao, mol.n_elec // 2), mol.hf_init()
    n = ham.nbqbits
    hf = int(hf) if np.isscalar(hf) else int(sum(1 << (n - 1 - q) for q, v in enumerate(hf) if v))
    theta = np.random.default_rng(2).uniform(-0.2, 0.2, len(gens))
    xs, zs, cs = pack_terms(n, ham.terms)
    cs = np.ascontiguousarray(cs.real)
    const = complex(ham.constant_coeff or 0.0).real
    with Statevector(n) as sv:
        sv.set_hamiltonian(ham)
        sv.set_ucc_program(gens, hf)
        exact = sv.energy(theta)
        t0 = time.perf_counter()
        plan = sv.measurement_groups()
        plan_ms = 1e3 * (time.perf_counter() - t0)
        for shots in shot_counts:
            for _ in range(3):
                sv.energy_sampled(theta, shots, seed=1)
            walls, values = [], []
            for r in range(reps):
                t0 = time.perf_counter()
                values.append(sv.energy_sampled(theta, shots, seed=1 + r))
                walls.append(1e6 * (time.perf_counter() - t0))
            info = sv.measure_info()
            prep = []
            for _ in range(reps):
                t0 = time.perf_counter()
                sv.prepare_state(theta)
                sv.norm2()                       # (a call that waits for the stream)
                prep.append(1e6 * (time.perf_counter() - t0))
            host_walls, host_values = [], []
            for r in range(host_reps):
                t0 = time.perf_counter()
                psi = sv.get_state()
                host_values.append(host_estimate(psi, n, xs, zs, cs, const, plan, shots, 1 + r))
                host_walls.append(1e6 * (time.perf_counter() - t0))
            rec = {"case": "H2O/STO-3G UCCSD", "qubits": n, "terms": int(len(xs)), "parameters": int(len(gens)), "groups": int(len(plan[1])),
                   "shots_per_group": shots, "exact_energy": exact, "plan_ms_first_call": plan_ms,
                   "device_wall_us_median": float(np.median(walls)), "device_wall_us_min": float(np.min(walls)), "measure_info": info,
                   "prepare_state_wall_us_median": float(np.median(prep)),
                   "host_wall_us_median": float(np.median(host_walls)), "host_over_device": float(np.median(host_walls) / np.median(walls)),
                   "device_first": values[0], "host_first": host_values[0],
                   "energies_mean_minus_exact": float(np.mean([v[0] for v in values]) - exact),
                   "energies_std": float(np.std([v[0] for v in values], ddof=1)), "std_error_mean": float(np.mean([v[1] for v in values]))}
            print(json.dumps(rec), flush=True)
            if out_dir:
                os.makedirs(out_dir, exist_ok=True)
                with open(os.path.join(out_dir, f"shot_noise_{shots}.json"), "w") as f:
                    json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
