"""Subspace-expansion matrices of a UCCSD state: ovqe_subspace_matrices (Statevector.subspace_matrices) against the only route the
library offered before it for the same matrices on the same state — m x apply_pauli_sum(O_j) into device buffers, m x
apply_pauli_sum(H) on them, and m (m + 1) x vec_dot for the upper triangles of S and Phi^H Sigma (the constant added on the host).
  python tools/exp_subspace.py [--case H2O|synth12] [--reps N] [--loop-reps N] [--out DIR]
H2O: H2O/STO-3G, 14 qubits, identity + 140 excitations.  synth12: fermion.synthetic_molecule(6, 3, 11), 12 qubits, identity + 117.
Both on the UCCSD state at theta ~ U(-0.2, 0.2), seed 2.  Times: HIP events of ovqe_subspace_info per stage and wall clock around the
synchronous call, medians after a warm-up; wall clock of the loop (median of --loop-reps).  One JSON line (and DIR/subspace_<case>.json)."""
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
    import torch
    from openvqe_amd import chem, excited, fermion
    from openvqe_amd.backend import Statevector
    from openvqe_amd.operators import pack_terms
    case, reps, loop_reps, out_dir = _arg("--case", "H2O"), _arg("--reps", 21), _arg("--loop-reps", 3), _arg("--out", "")
    if case == "synth12":
        n_spatial, n_occ = 6, 3
        ham, gens, hf = fermion.synthetic_molecule(n_spatial, n_occ, 11)
    else:
        mol = chem.molecule(case)
        mol.rhf()
        n_spatial, n_occ = mol.nao, mol.n_elec // 2
        ham, gens, hf = mol.jw_hamiltonian(), fermion.uccsd_generators(n_spatial, n_occ), mol.hf_init()
    n = ham.nbqbits
    ops = excited.excitation_operators(n_spatial, n_occ)
    m = len(ops)
    theta = np.random.default_rng(2).uniform(-0.2, 0.2, len(gens))
    med = lambda v: float(np.median(v))   # noqa: E731
    with Statevector(n) as sv:
        sv.set_hamiltonian(ham)
        sv.set_ucc_program(gens, hf)
        sv.prepare_state(theta)
        for _ in range(3):   # warm-up: buffers, code objects
            G, S = sv.subspace_matrices(ops, raw=True)
        wall, infos = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            G, S = sv.subspace_matrices(ops, raw=True)
            wall.append(time.perf_counter() - t0)
            infos.append(sv.subspace_info())
        # ---- the loop over the unit operations
        packed = sv._pack_pool_with_constants(ops)
        offsets, xs, zs, cre, cim = packed
        hx, hz, hc = pack_terms(n, ham.terms)
        phi = torch.zeros((m, 1 << n), dtype=torch.complex128, device="cuda")
        sig = torch.zeros((m, 1 << n), dtype=torch.complex128, device="cuda")
        torch.cuda.synchronize()
        row = (1 << n) * 16
        loop_wall = []
        for _ in range(loop_reps + 1):
            t0 = time.perf_counter()
            for j in range(m):
                a, b = int(offsets[j]), int(offsets[j + 1])
                sv.apply_pauli_sum(xs[a:b], zs[a:b], cre[a:b] + 1j * cim[a:b], phi.data_ptr() + j * row)
            for j in range(m):
                sv.apply_pauli_sum(hx, hz, hc, sig.data_ptr() + j * row, ket_ptr=phi.data_ptr() + j * row)
            S2 = np.zeros((m, m), np.complex128)
            G2 = np.zeros((m, m), np.complex128)
            for i in range(m):
                for j in range(i, m):
                    S2[i, j] = sv.vec_dot(phi.data_ptr() + i * row, phi.data_ptr() + j * row)
                    G2[i, j] = sv.vec_dot(phi.data_ptr() + i * row, sig.data_ptr() + j * row)
            G2 += float(np.real(ham.constant_coeff)) * S2
            loop_wall.append(time.perf_counter() - t0)
        loop_wall = loop_wall[1:]
    iu = np.triu_indices(m)
    info = infos[-1]
    res = {"case": case, "qubits": n, "m": m, "h_terms": len(ham.terms), "info": info,
           "rows_us": med([i["rows_us"] for i in infos]), "expand_us": med([i["expand_us"] for i in infos]),
           "sigma_us": med([i["sigma_us"] for i in infos]), "gram_us": med([i["gram_us"] for i in infos]),
           "call_wall_us": 1e6 * med(wall), "call_wall_min_us": 1e6 * float(np.min(wall)), "reps": reps,
           "loop_wall_us": 1e6 * med(loop_wall), "loop_reps": loop_reps, "loop_calls": 2 * m + m * (m + 1),
           "max_abs_dS_vs_loop": float(np.abs(S[iu] - S2[iu]).max()), "max_abs_dG_vs_loop": float(np.abs(G[iu] - G2[iu]).max()),
           "max_abs_G_minus_GH": float(np.abs(G - G.conj().T).max())}
    res["loop_over_call"] = res["loop_wall_us"] / res["call_wall_us"]
    print(json.dumps(res), flush=True)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, f"subspace_{case}.json"), "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
