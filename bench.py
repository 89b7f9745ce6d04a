#!/usr/bin/env python3
"""bench.py — headline benchmark of the statevector backend (contract: see the task prompt).

Metric (BASELINE.json): VQE energy evaluations / second on the H2O/STO-3G-shaped UCCSD problem
(14 qubits, 140 generators = 1000 Pauli rotations, JW Hamiltonian), plus achieved HBM GB/s of the
single-Pauli-string sweep at 30 qubits against the 8 TB/s roofline.

A "step" = one batch of B parameter vectors pushed through the whole hot path (|HF> -> 1000 Pauli
rotations -> <psi|H|psi>), i.e. B energy evaluations; all inputs (program, Hamiltonian, the B x K
parameter blocks) are resident in HBM before the timed region; the B energies of a step are copied
back to the host inside the step.  With N GPUs every rank evaluates its own
batch of B vectors (replicas over the batch dimension, no data-path collective): weak scaling.

A plain run sets up, warms up, times --steps steps and prints the line (`ms_per_step` = wall time of one timed step);
--dump-outputs DIR also writes the energies of the last timed step.  Everything else (the dense-kernel cross-check, the
sharded block, the 30-qubit HBM roofline sweeps, the side workloads and the CPU baseline with its oracle check of the timed
batch) runs only with --full.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E peak (MI355X_MICROARCH.md)
LDS_PEAK_GBS = 150000.0  # aggregate LDS read rate, every CU streaming ds_read_b64/b128 (MI355X_MICROARCH.md, LDS)


def build_workload():
    """H2O/STO-3G at the reference's geometry (ref:openvqe/common_files/molecule_factory.py:138-148): integrals, RHF
    and the Jordan-Wigner Hamiltonian from the in-repo front-end (no PySCF / myQLM on the GPU box), all-electron
    UCCSD generators (5 occupied, 2 virtual spatial orbitals: 140 generators = 1000 Pauli rotations)."""
    from openvqe_amd import chem, fermion
    mol = chem.molecule("H2O")
    mol.rhf()
    ham = mol.jw_hamiltonian()
    gens = fermion.uccsd_generators(mol.nao, mol.n_elec // 2)
    return ham, gens, mol.hf_init()


def m1_strings(n):
    """SURVEY.md §8d M1 string set (reference qubit numbering, 0 = MSB)."""
    def s(op, qs):
        return op, qs
    out = [
        ("XXXY@0-3", s("XXXY", [0, 1, 2, 3])),
        ("XXXY@low", s("XXXY", [n - 4, n - 3, n - 2, n - 1])),
        ("YXXX@spread", s("YXXX", [0, (n - 1) // 3, 2 * (n - 1) // 3, n - 1])),
        ("JWsingle", s("X" + "Z" * (n - 2) + "Y", list(range(n)))),
        ("JWdouble", s("XX" + "Z" * (n - 7) + "XY", [2, 3] + list(range(4, n - 3)) + [n - 3, n - 2])),
        ("allZ", s("Z" * n, list(range(n)))),
        ("Z@mid", s("Z", [n // 2])),
    ]
    rng = np.random.default_rng(7)
    for k in range(9):
        qs = [q for q in range(n) if rng.random() < 0.5] or [0]
        op = "".join(rng.choice(list("XYZ"), len(qs)))
        out.append((f"rand{k}", s(op, qs)))
    return out


def roofline_leg(device, n, reps=20, warmup=3):
    """single-Pauli-string sweep at n qubits: HIP-event timing inside the library, per string."""
    from openvqe_amd.backend import Statevector
    from openvqe_amd.operators import pack_string
    res = []
    with Statevector(n, device=device) as sv:
        sv.randomize(20250227)
        for name, (op, qs) in m1_strings(n):
            x, z = pack_string(n, op, qs)
            ms = sv.time_pauli_rotation(x, z, 0.1, warmup=warmup, reps=reps)
            res.append({"string": name, "ms": ms, "GBs": 32.0 * (1 << n) / (ms * 1e-3) / 1e9, "diag": x == 0})
    return res


def extra_workloads_leg(device):
    """SURVEY §8d M2 side figures (not `value`): single-evaluation latency, one finite-difference gradient
    (B = K+1) and a large batch for H2 (4 qubits), LiH (12) and H2O (14), all STO-3G UCCSD from the in-repo front-end."""
    from openvqe_amd import chem, fermion
    from openvqe_amd.backend import Statevector
    out = []
    for name in ("H2-STO3G-WSSVQE", "LIH", "H2O"):
        mol = chem.molecule(name)
        mol.rhf()
        ham = mol.jw_hamiltonian()
        gens = fermion.uccsd_generators(mol.nao, mol.n_elec // 2)
        K = len(gens)
        rng = np.random.default_rng(K)
        with Statevector(ham.nbqbits, device=device) as sv:
            sv.set_hamiltonian(ham)
            sv.set_ucc_program(gens, mol.hf_init())
            row = {"molecule": name, "qubits": ham.nbqbits, "generators": K,
                   "rotations": sum(len(g.terms) for g in gens), "hamiltonian_terms": len(ham.terms) + 1}
            for label, B, reps in (("single", 1, 300), ("fd_gradient", K + 1, 10), ("batch4096", 4096, 3)):
                th = rng.uniform(-0.1, 0.1, (B, K))
                sv.energy_batch(th)
                t0 = time.perf_counter()
                if B == 1:   # what scipy's optimisers call: ovqe_energy, one parameter vector per call
                    for _ in range(reps):
                        sv.energy(th[0])
                else:
                    for _ in range(reps):
                        sv.energy_batch(th)
                dt = (time.perf_counter() - t0) / reps
                row[label] = {"B": B, "ms": 1e3 * dt, "evals_per_s": B / dt}
            out.append(row)
    out.extend(gate_and_midsize_workloads(device))
    return out


def _quccsd_gates(m, o, stride=1):
    from openvqe_amd.common_files.circuit import quccsd_gate_list
    return quccsd_gate_list(m, o, stride)


def gate_and_midsize_workloads(device):
    """configs[3]-type side figures: the QUCCSD gate list at H2O size (literal execution vs Clifford-frame form) and
    24-qubit state preparation (QUCCSD gate list; UCCSD Pauli-rotation program) on the streaming kernels with
    LDS-tiled multi-op sweeps, against one sweep per op."""
    from openvqe_amd import chem, fermion
    from openvqe_amd.backend import Statevector
    out = []
    mol = chem.molecule("H2O")
    mol.rhf()
    ham = mol.jw_hamiltonian()
    gates, K, hf = _quccsd_gates(mol.nao, mol.n_elec // 2)
    rng = np.random.default_rng(5)
    row = {"workload": "H2O/STO-3G QUCCSD gate list", "qubits": ham.nbqbits, "literal_gates": len(gates), "parameters": K}
    with Statevector(ham.nbqbits, device=device) as sv:
        sv.set_hamiltonian(ham)
        th_all = rng.uniform(-0.1, 0.1, (4096, K))
        for label, mode, B in (("literal", 0, 64), ("clifford_frame", 1, 4096)):
            sv.set_option("clifford_frame", mode)
            sv.set_gate_program(gates, K, hf)
            th = th_all[:B]
            e0 = sv.energy_batch(th[:4])
            sv.energy_batch(th)
            t0 = time.perf_counter()
            sv.energy_batch(th)
            dt = time.perf_counter() - t0
            row[label] = {"B": B, "evals_per_s": B / dt, "program": sv.program_info(), "E0": float(e0[0])}
    out.append(row)
    # H2O/STO-3G: the pieces of the ADAPT / gradient-based flows around the energy evaluation
    from openvqe_amd import pools
    from openvqe_amd.backend import GRAD_FERMIONIC
    gens = fermion.uccsd_generators(mol.nao, mol.n_elec // 2)
    _, pool = pools.spin_complement_gsd(mol.n_elec, mol.nao)
    th1 = rng.uniform(-0.1, 0.1, len(gens))
    flows = {"workload": "H2O/STO-3G flow pieces", "qubits": ham.nbqbits}
    with Statevector(ham.nbqbits, device=device) as sv:
        sv.set_hamiltonian(ham)
        sv.set_ucc_program(gens, mol.hf_init())

        def timed(fn, reps=5):
            fn()
            t0 = time.perf_counter()
            for _ in range(reps):
                r = fn()
            return 1e3 * (time.perf_counter() - t0) / reps, r

        ms, (e, g) = timed(lambda: sv.energy_gradient(th1))
        flows["adjoint_gradient_all_parameters"] = {"ms": ms, "parameters": len(gens), "energy": float(e)}
        sv.prepare_state(th1)
        ms, gr = timed(lambda: sv.pool_gradients(pool, GRAD_FERMIONIC))
        flows["adapt_gradient_screen"] = {"ms": ms, "pool_operators": len(pool), "norm": float(np.linalg.norm(gr))}
        ms, (e0, resid, its) = timed(lambda: sv.ground_state(tol=1e-10), reps=2)
        flows["ground_state_lanczos"] = {"ms": ms, "energy": float(e0), "residual": float(resid), "steps": int(its)}
    out.append(flows)
    m, o, stride = 12, 5, 5
    n = 2 * m
    gates, K, hf = _quccsd_gates(m, o, stride)
    gens = fermion.uccsd_generators(m, o)[::stride]
    theta = rng.uniform(-0.1, 0.1, K)
    row = {"workload": "24-qubit state preparation (every 5th UCCSD excitation of 10e/12o)", "qubits": n,
           "excitations": K, "literal_gates": len(gates), "pauli_rotations": sum(len(g.terms) for g in gens)}
    with Statevector(n, device=device) as sv:
        for label, setter, frame, bits in (
                ("quccsd_literal_one_sweep_per_gate", lambda: sv.set_gate_program(gates, K, hf), 0, 0),
                ("quccsd_literal_tiled", lambda: sv.set_gate_program(gates, K, hf), 0, -1),
                ("quccsd_clifford_frame_tiled", lambda: sv.set_gate_program(gates, K, hf), 1, -1),
                ("uccsd_one_sweep_per_run", lambda: sv.set_ucc_program(gens, hf), 1, 0),
                ("uccsd_tiled", lambda: sv.set_ucc_program(gens, hf), 1, -1)):
            sv.set_option("clifford_frame", frame)
            sv.set_option("tile_bits", bits)
            setter()
            sv.prepare_state(theta)
            t0 = time.perf_counter()
            sv.prepare_state(theta)
            dt = time.perf_counter() - t0
            info = sv.program_info()
            row[label] = {"ms": 1e3 * dt, "sweeps": info["sweeps"], "tiled_sweeps": info["tiled_sweeps"]}
    out.append(row)
    # the whole 24-qubit molecule-shaped UCCSD evaluation (1715 generators = 13300 rotations, 29736-term
    # JW Hamiltonian / 5479 x-groups) on the streaming path: real-amplitude tile sweeps + tiled <H>; from the second call
    # on through the sector path (circuit and materialised <H> on the support of the program's states, profiles/r2_sector);
    # the same handle with the sector path off = the compact cover of profiles/r2_n24
    ham24, gens24, hf24 = fermion.synthetic_molecule(m, o, seed=24)
    th24 = rng.uniform(-0.1, 0.1, len(gens24))
    row24 = {"workload": "24-qubit UCCSD energy evaluation (SURVEY 8d M3)", "qubits": n, "generators": len(gens24),
             "rotations": sum(len(g.terms) for g in gens24), "hamiltonian_terms": len(ham24.terms) + 1,
             "x_groups": len(set(ham24.packed()[0].tolist()))}
    b_eval = 32.0 * (1 << n) * row24["rotations"] + 16.0 * (1 << n) * row24["x_groups"]
    for label, sector in (("sector_path", 1), ("dense_state_compact_cover", 0)):
        with Statevector(n, device=device) as sv:
            sv.set_option("sector", sector)
            sv.set_hamiltonian(ham24)
            sv.set_ucc_program(gens24, hf24)
            times = []
            for _ in range(6):
                t0 = time.perf_counter()
                e24 = sv.energy(th24)
                times.append(1e3 * (time.perf_counter() - t0))
            info = sv.program_info()
            row24[label] = {"ms_first_call_dense": times[0], "ms_second_call_builds_tables": times[1],
                            "ms_steady_state": min(times[2:]), "energy": float(e24),
                            "algorithmic_GBs": b_eval / (min(times[2:]) * 1e-3) / 1e9, "program": info}
            if sector:
                row24["ms_steady_state"] = min(times[2:])
                row24[label]["table_GB"] = info["sector_bytes"] / 1e9
                # the path's two kernels under HIP events (on the handle's stream): circuit sweeps, <H> table stream
                sv.set_option("sector_profile", 1)
                circ_us, exp_us = [], []
                for _ in range(5):
                    sv.energy(th24)
                    pi = sv.program_info()
                    circ_us.append(pi["sector_circuit_us"])
                    exp_us.append(pi["sector_expect_us"])
                sv.set_option("sector_profile", 0)
                hb = sv.program_info()["sector_h_stream_bytes"]
                t_exp = 1e-6 * float(np.mean(exp_us))
                row24[label]["roofline_expect_kernel"] = {
                    "bound": "hbm", "kernel": "k_sector_expect (materialised <H>: one pass over the table per evaluation)",
                    "achieved": hb / t_exp / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": hb / t_exp / 1e9 / HBM_PEAK_GBS,
                    "bytes_per_launch": hb, "avg_launch_ms": 1e3 * t_exp,
                    "traffic_source": newest_profile("*_sector", "pmc_summary.txt") + " (FETCH_SIZE x2)"}
                row24[label]["circuit_sweeps_ms"] = 1e-3 * float(np.mean(circ_us))
            if sector:
                # batched evaluations on the tables (what a finite-difference gradient of the reference's BFGS submits)
                thb = rng.uniform(-0.1, 0.1, (64, len(gens24)))
                sv.energy_batch(thb)
                t0 = time.perf_counter()
                eb = sv.energy_batch(thb)
                dtb = (time.perf_counter() - t0) / 64
                row24[label]["batch_64"] = {"ms_per_evaluation": 1e3 * dtb, "x_serial_rate": min(times[2:]) * 1e-3 / dtb,
                                            "max_abs_diff_vs_single": float(max(abs(eb[k] - sv.energy(thb[k])) for k in (0, 63)))}
            # exact gradient of all parameters (adjoint method; on the sector tables when they exist)
            tg = []
            for _ in range(2):
                t0 = time.perf_counter()
                _, g24 = sv.energy_gradient(th24)
                tg.append(1e3 * (time.perf_counter() - t0))
            row24[label]["ms_gradient_all_parameters"] = min(tg)
            row24[label]["gradient_norm"] = float(np.linalg.norm(g24))
    out.append(row24)
    # BASELINE.json configs[3] on its molecule: N2 / cc-pVDZ, (10 electrons, 12 orbitals) active space = 24 qubits, from the
    # in-repo front-end (d-shell integrals, RHF, frozen core).  UCCSD (JW generators in the reference's operator order) at
    # the MP2 amplitudes, and the reference's QUCCSD gate list (Clifford-frame form) on the same operators.
    from openvqe_amd import chem
    from openvqe_amd.common_files.circuit import quccsd_gate_list
    mol = chem.molecule("N2-CCPVDZ")
    e_rhf = mol.rhf()
    prob = chem.cas_problem(mol, 2, 12)
    hamn = prob.jw_hamiltonian()
    size, cluster_ops, spin_ops, theta_mp2, hfn = prob.uccsd()
    rown = {"workload": "N2/cc-pVDZ (10e,12o) active space, 24 qubits (configs[3])", "qubits": prob.nbqbits,
            "E_RHF": e_rhf, "E_MP2": mol.mp2_energy(), "cluster_operators": size, "hamiltonian_terms": len(hamn.terms) + 1,
            "x_groups": len(set(hamn.packed()[0].tolist()))}
    with Statevector(prob.nbqbits, device=device) as sv:
        t_su = time.perf_counter()
        sv.set_hamiltonian(hamn)
        t_h = time.perf_counter() - t_su
        sv.set_ucc_program(spin_ops, hfn)
        t_p = time.perf_counter() - t_su - t_h
        times = []
        for _ in range(6):
            t0 = time.perf_counter()
            e_ucc = sv.energy(theta_mp2)
            times.append(1e3 * (time.perf_counter() - t0))
        # time to the first energy THAT COMES FROM THE TABLES: Hamiltonian + program + every evaluation up to and including the one
        # that built them (the process is warm: the library's code objects were loaded by the workloads above)
        built = 1 if times[1] < 3.0 * min(times[2:]) else 2
        rown["uccsd_at_theta_mp2"] = {"energy": float(e_ucc), "ms_first_call": times[0], "ms_second_call_builds_tables": times[1],
                                      "ms_steady_state": min(times[2:]),
                                      "setup_ms": {"set_hamiltonian": 1e3 * t_h, "set_program": 1e3 * t_p,
                                                   "evaluations_until_tables": built, "evaluations_ms": float(sum(times[:built])),
                                                   "total": 1e3 * (t_h + t_p) + float(sum(times[:built]))},
                                      "program": sv.program_info()}
        # ... and the optimisation itself: L-BFGS-B from the MP2 amplitudes with the exact gradient (adjoint pass on the
        # sector tables), to |g|_inf < 1e-6
        from scipy.optimize import minimize
        calls = []

        def fun(th):
            t0 = time.perf_counter()
            e, g = sv.energy_gradient(th)
            calls.append(time.perf_counter() - t0)
            return e, g

        t0 = time.perf_counter()
        from openvqe_amd.common_files.host_threads import one_blas_thread   # the optimiser's vectors on one BLAS thread (what the mirrors do)
        with one_blas_thread():
            res = minimize(fun, np.array(theta_mp2), jac=True, method="L-BFGS-B", options={"maxiter": 100, "gtol": 1e-6, "ftol": 1e-14})
        rown["uccsd_vqe_lbfgs_exact_gradient"] = {"energy": float(res.fun), "iterations": int(res.nit), "gradient_calls": len(calls),
                                                  "max_abs_gradient": float(np.abs(res.jac).max()),
                                                  "wall_s": time.perf_counter() - t0,
                                                  "ms_per_gradient_call_steady": 1e3 * float(np.median(calls[2:])) if len(calls) > 2 else None,
                                                  "program": sv.program_info()}
        t0 = time.perf_counter()
        e_fci, r_fci, it_fci = sv.sector_ground_state(tol=1e-10)
        rown["fci_of_the_sector_lanczos"] = {"energy": e_fci, "residual": r_fci, "iterations": it_fci, "determinants": 792 ** 2,
                                             "wall_s": time.perf_counter() - t0,
                                             "uccsd_minus_fci": float(res.fun) - e_fci}
        gates, K, _ = quccsd_gate_list(12, 5, 1, excitations=[op.terms[0].qbits for op in cluster_ops])
        t_su = time.perf_counter()
        sv.set_gate_program(gates, K, hfn)
        t_pq = time.perf_counter() - t_su
        sv.set_option("sector_profile", 1)
        times, circ_us, exp_us = [], [], []
        for _ in range(8):
            t0 = time.perf_counter()
            e_q = sv.energy(theta_mp2)
            times.append(1e3 * (time.perf_counter() - t0))
            inf = sv.program_info()
            if inf["sector_expect_us"] > 0:
                circ_us.append(inf["sector_circuit_us"])
                exp_us.append(inf["sector_expect_us"])
        sv.set_option("sector_profile", 0)
        infq = sv.program_info()
        if exp_us:
            # configs[3] as written, per kernel (HIP events on the handle's stream around the two halves of an evaluation): the
            # materialised <H> streams its table from HBM; the circuit sweeps keep the 32-MiB state in the caches and move it
            # through LDS — their HBM-side traffic is the committed PMC profile's (profiles/r4_quccsd24)
            t_e, t_c = float(np.mean(exp_us[1:] or exp_us)) * 1e-6, float(np.mean(circ_us[1:] or circ_us)) * 1e-6
            nsw, sup = infq["sector_sweeps"], infq["sector_support"]
            rown["roofline_quccsd24"] = {
                "expect_kernel": {"bound": "hbm", "kernel": "k_sector_expect<512>", "achieved": infq["sector_h_stream_bytes"] / t_e / 1e9,
                                  "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": infq["sector_h_stream_bytes"] / t_e / 1e9 / HBM_PEAK_GBS,
                                  "bytes_per_launch": infq["sector_h_stream_bytes"], "avg_launch_ms": 1e3 * t_e},
                "circuit_sweeps": {"bound": "lds", "kernel": "k_sector_sweep_reg<256> (regular support: sweeps from bit arithmetic, no pair words)"
                                   if infq["sector_regular_slot_bits"] else "k_sector_sweep<1024> (pair words)",
                                   "launches": nsw, "avg_launch_ms": 1e3 * t_c / max(nsw, 1), "ms_per_evaluation": 1e3 * t_c,
                                   "hbm_side_bytes_per_launch_algorithmic": 20 * sup if infq["sector_regular_slot_bits"] else None,
                                   "hbm_side_GBs": (20 * sup * nsw / t_c / 1e9) if infq["sector_regular_slot_bits"] else None,
                                   "note": "8 B read + 8 B written per amplitude and sweep + 4 B of gather index; the ops of a sweep "
                                           "(46 on average) act on the tile in LDS"},
                "traffic_source": newest_profile("*quccsd24", "pmc_summary.txt") + " (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes)"}
        calls = []
        t0 = time.perf_counter()
        with one_blas_thread():
            resq = minimize(fun, np.array(theta_mp2), jac=True, method="L-BFGS-B", options={"maxiter": 100, "gtol": 1e-6, "ftol": 1e-14})
        rown["quccsd_vqe_lbfgs_exact_gradient"] = {"energy": float(resq.fun), "iterations": int(resq.nit), "gradient_calls": len(calls),
                                                   "max_abs_gradient": float(np.abs(resq.jac).max()),
                                                   "wall_s": time.perf_counter() - t0,
                                                   "ms_per_gradient_call_steady": 1e3 * float(np.median(calls[2:])) if len(calls) > 2 else None}
        built = 1 if times[1] < 3.0 * min(times[2:]) else 2
        rown["quccsd_gate_list_at_theta_mp2"] = {"literal_gates": len(gates), "energy": float(e_q), "ms_first_call": times[0],
                                                 "ms_steady_state": min(times[2:]),
                                                 "setup_ms": {"set_gate_program": 1e3 * t_pq, "evaluations_until_tables": built,
                                                              "evaluations_ms": float(sum(times[:built])),
                                                              "total": 1e3 * t_pq + float(sum(times[:built]))},
                                                 "program": sv.program_info()}
    # the ADAPT side of the same molecule: screen state of five spin-adapted generators (exact exponentials), the screen
    # over the 665-operator singlet pool, and sigma = H psi / the fun_fidelity reference vector over the whole register
    from openvqe_amd import pools
    from openvqe_amd.backend import GRAD_FERMIONIC
    _, _, singlets = pools.singlet_sd(10, 12)
    with Statevector(prob.nbqbits, device=device) as sv:
        sv.set_hamiltonian(hamn)
        adapt = {"pool_operators": len(singlets)}
        for label, den in (("support", 16), ("register", 0)):
            sv.set_option("screen_sparse", den)
            t_exp, t_scr = [], []
            for rep in range(3):
                sv.init_basis(hfn)
                t0 = time.perf_counter()
                for k, th in zip((3, 200, 411, 77, 640), (0.2, -0.15, 0.1, 0.3, -0.25)):
                    sv.apply_exp_pauli_sum(singlets[k], th)
                sv.norm2()
                t_exp.append(1e3 * (time.perf_counter() - t0) / 5)
                t0 = time.perf_counter()
                g = sv.pool_gradients(singlets, GRAD_FERMIONIC)
                t_scr.append(1e3 * (time.perf_counter() - t0))
            adapt[label] = {"exact_exponential_ms_per_operator": min(t_exp), "screen_ms": min(t_scr),
                            "amplitudes_walked_by_the_screen": sv.last_screen_support(),
                            "largest_gradient": float(np.abs(g).max())}
        t0 = time.perf_counter()
        e_g, r_g, it_g = sv.ground_state(tol=1e-10)
        adapt["reference_vector_lanczos_whole_register"] = {"energy": e_g, "residual": r_g, "iterations": it_g,
                                                            "wall_s": time.perf_counter() - t0}
        rown["fermionic_adapt_phases"] = adapt
    # ... and the loop itself: 30 macro-iterations of the fermionic-ADAPT mirror (ref:openvqe/adapt/fermionic_adapt_vqe.py:371-593) on
    # this molecule — COBYLA over the growing ansatz (about 14 000 energy evaluations), the screen over the 665-operator pool, the
    # fidelity against the sector's ground vector (the mirror's SECTOR_GROUND_SPACE opt-in: the reference diagonalises the dense 2^24
    # matrix, which nothing can do) — wall time with every table build inside
    from openvqe_amd.adapt import fermionic_adapt_vqe as fav
    from openvqe_amd import evaluator as _ev
    saved_flag, fav.SECTOR_GROUND_SPACE = getattr(fav, "SECTOR_GROUND_SPACE", False), True
    saved_disp, fav._FLAVOUR.optimiser_display = fav._FLAVOUR.optimiser_display, False   # (COBYLA's own report comes from Fortran's
    # buffered unit 6 and would surface at process exit, behind the JSON line)
    sys.stdout.flush()
    fd_out = os.dup(1)
    devnull = os.open(os.devnull, os.O_WRONLY)
    try:
        os.dup2(devnull, 1)    # the mirror prints the reference's per-iteration report, COBYLA its own (from Fortran)
        t0 = time.perf_counter()
        trace, _ = fav.fermionic_adapt_vqe(None, None, None, hamn, singlets, hfn, 1, -109.0745445341, "COBYLA", 1e-6, "norm", 1e-3, 30)
        wall = time.perf_counter() - t0
    finally:
        sys.stdout.flush()
        os.dup2(fd_out, 1)
        os.close(fd_out)
        os.close(devnull)
        fav.SECTOR_GROUND_SPACE = saved_flag
        fav._FLAVOUR.optimiser_display = saved_disp
        _ev.release_backends()
        import openvqe_amd.qat_compat as _qc
        for _sv in list(fav._screens.values()) + (list(_qc._default_qpu._sv.values()) if _qc._default_qpu else []):
            _sv.close()
        fav._screens.clear(); fav._evaluators.clear()
        _qc._default_qpu = None
    energies = [float(e) for e in trace.get("energies", [])] if isinstance(trace, dict) else []
    rown["fermionic_adapt_30_iterations"] = {"wall_s": wall, "iterations": len(energies), "energy_last": energies[-1] if energies else None,
                                             "energy_first": energies[0] if energies else None}
    out.append(rown)
    return out


XGMI_LINK_GBS = 153.0  # one xGMI link, one direction (task brief / MI355X platform: 7 links x ~153 GB/s per GPU)


def two_body_string(rng, n):
    """(x, z) of a JW double-excitation-like string: X/Y on 4 random qubits, Z chains between the pairs (index-bit masks)"""
    q = sorted(rng.choice(n, 4, replace=False).tolist())
    x = sum(1 << (n - 1 - k) for k in q)
    z = 0
    for lo, hi in ((q[0], q[1]), (q[2], q[3])):
        for k in range(lo + 1, hi):
            z |= 1 << (n - 1 - k)
    ys = rng.choice(4, int(rng.choice([1, 3])), replace=False)
    for k in ys:
        z |= 1 << (n - 1 - q[k])
    return x, z


def sharded_workload(n, rotations=64, terms=1000, seed=34):
    """configs[4]: `rotations` JW two-body Pauli rotations and a `terms`-term random JW Hamiltonian
    (30 % diagonal strings, even number of Y: real symmetric) on n qubits -> (xs, zs, phis, hx, hz, hc)"""
    rng = np.random.default_rng(seed)
    rots = [two_body_string(rng, n) for _ in range(rotations)]
    xs, zs = [r[0] for r in rots], [r[1] for r in rots]
    phis = rng.uniform(-0.2, 0.2, rotations)
    hx, hz = [], []
    for _ in range(terms):
        x, z = two_body_string(rng, n)
        if rng.random() < 0.3:
            x = 0  # diagonal term
        else:
            z ^= x & z if rng.random() < 0.5 else 0
            if bin(x & z).count("1") & 1:   # keep H real-symmetric: even number of Y
                z ^= x & -x
        hx.append(x); hz.append(z)
    hc = rng.normal(size=terms)
    return xs, zs, phis, hx, hz, hc


SHARDED_SEED = 20250227
# Energies of the sharded workload that are on record: (qubits, rotations, terms) -> <H> after the rotations.  The synthetic state is
# defined per GLOBAL index and the operators per qubit count, so the value cannot depend on the number of GPUs; any N compares its
# strong leg (and its weak leg where a value is on record) with these to 1e-11 |H|_1.  Source: profiles/r4b/bench.json (1 GPU, 31 q);
# confirmed by the C oracle on a 32-GiB host state (tests/oracle_sharded_energy.py, profiles/r6_oracle31/: 0.0006064921993098272,
# 7.4e-18 |H|_1 away).
SHARDED_KNOWN = {(31, 64, 1000): 0.0006064921993039994}


def sharded_leg(n, local_rank, world, rank, rotations=64, terms=1000, barrier=None, dry_rank=None, real_state=False):
    """One pass of configs[4] over the index-bit-partitioned register (openvqe_amd.distributed): the synthetic state
    (recomputable on the host per global index, openvqe_amd/synth.py) -> `rotations` Pauli rotations (half-shard
    exchanges over RCCL for X/Y on global qubits) -> <H> (partner-shard reads for global-x groups).  World size 1 runs
    the same code on one shard.  -> dict (identical on every rank up to the timings, which are this rank's)."""
    import torch
    from openvqe_amd.distributed import ShardedStatevector
    g = world.bit_length() - 1
    xs, zs, phis, hx, hz, hc = sharded_workload(n, rotations, terms)
    sv = ShardedStatevector(n, device=local_rank, dry_rank=dry_rank)
    if dry_rank is not None:
        world, rank = dry_rank
        g = world.bit_length() - 1
    if os.environ.get("OVQE_BENCH_SINGLE_DEVICE") and world > 1 and dry_rank is None:
        # every rank's shard sits on device 0: compute sections take the device one rank at a time, so that their seconds are a rank's own
        sv.compute_lock = os.path.join("/tmp", "ovqe_bench_compute_%s.lock" % os.environ.get("MASTER_PORT", "0"))
    sv.randomize(SHARDED_SEED)
    if real_state:
        # the workload's rotation strings all carry an odd number of Y — what every UCC / ADAPT generator does — so a REAL state stays
        # real: the real parts of the synthetic state, renormalised, on float64 shards (8-byte amplitudes: half the bytes of every sweep)
        sv.engine.set_real(True)
        sv.real = True
        sv.engine.tensor.mul_(1.0 / sv.norm2() ** 0.5)
    stall = os.environ.get("OVQE_BENCH_INJECT_STALL_RANK")      # tests: this rank never posts its half of the first exchange
    if stall is not None and int(stall) == rank:
        time.sleep(10 ** 6)
    if os.environ.get("OVQE_BENCH_INJECT_SHARDED_ERROR"):        # tests: the leg fails on every rank (what a collective's error does)
        raise RuntimeError("injected failure of the sharded leg")

    from openvqe_amd.distributed import _progress

    def fence():
        _progress("barrier between the phases of the sharded leg")
        torch.cuda.synchronize()
        if barrier is not None:
            barrier()
            torch.cuda.synchronize()
        _progress("local sweeps")

    fence()
    t0 = time.perf_counter()
    sv.apply_pauli_rotations(xs, zs, phis)
    fence()
    t_rot = time.perf_counter() - t0
    st = dict(sv.stats)
    cnt = dict(sv.engine.counters)
    t0 = time.perf_counter()
    e = sv.expectation(hx, hz, hc, 0.0)
    fence()
    t_exp = time.perf_counter() - t0
    n2 = sv.norm2()
    st2 = dict(sv.stats)
    cnt2 = dict(sv.engine.counters)
    groups = len(set(hx))
    swap_bytes = st["bytes_sent"]
    read_bytes = st2["bytes_sent"] - st["bytes_sent"]
    t_local = max(st["local_sweeps_s"], 1e-9)
    info = sv.engine.sum_info(sv._plan_sum(sv._plan_for(hx, hz, hc, 0.0), "expect")) if hasattr(sv.engine, "sum_info") else {}
    link = XGMI_LINK_GBS * 1e9
    out = {
        "workload": f"{rotations} JW two-body rotations + {terms}-term random JW Hamiltonian ({groups} x-groups) on the "
                    f"synthetic {n}-qubit state, index-bit partition over {world} GPU(s)",
        "n_qubits": n, "n_gpus": world, "shard_GiB": 16.0 * 2 ** (n - g) / 2 ** 30,
        "rotations_s": t_rot, "ms_per_rotation": 1e3 * t_rot / rotations,
        "local_sweeps_s": t_local, "exchange_s": st["swap_s"],
        "swaps": st["swaps"], "exchange_pieces": st["pieces"], "exchanged_GiB_per_rank": swap_bytes / 2 ** 30,
        "xgmi_link_GBs_exchange": (swap_bytes / st["swap_s"] / 1e9) if st["swap_s"] > 0 else None,
        "xgmi_link_frac_of_153": (swap_bytes / st["swap_s"] / 1e9 / XGMI_LINK_GBS) if st["swap_s"] > 0 else None,
        # what the kernels did (this rank): the engine fuses same-x runs and takes several runs per LDS-tiled sweep, so the
        # launches that stream the shard are FEWER than the rotations — the bandwidth is bytes actually moved / time
        "local_sweeps_executed": cnt["rotation_passes"], "local_bytes_moved_per_rank": cnt["rotation_bytes"],
        "local_sweep_GBs_per_gpu": cnt["rotation_bytes"] / t_local / 1e9,
        "local_sweep_frac_of_hbm_peak": cnt["rotation_bytes"] / t_local / 1e9 / HBM_PEAK_GBS,
        # the same work priced at one full sweep per rotation / x-group over the whole register (a RATE OF WORK, not a bandwidth:
        # it exceeds the HBM peak whenever runs are fused)
        "rotations_per_s_equivalent_GBs_aggregate": 32.0 * 2 ** n * rotations / t_local / 1e9,
        "rotations_equivalent_GBs_aggregate_incl_exchange": 32.0 * 2 ** n * rotations / t_rot / 1e9,
        "expectation_s": t_exp, "full_shard_reads": st2["full_shard_reads"], "chunk_reads": st2["chunk_reads"],
        "partners_read_concurrently": st2["partners_per_read"],
        "shard_read_GiB_per_rank": read_bytes / 2 ** 30,
        "shard_read_wait_s": st2["shard_read_s"],
        "xgmi_GBs_shard_reads_all_links": (read_bytes / st2["shard_read_s"] / 1e9) if st2["shard_read_s"] > 0 else None,
        "xgmi_link_GBs_shard_reads": (read_bytes / st2["shard_read_s"] / 1e9 / max(1, st2["partners_per_read"]))
                                     if st2["shard_read_s"] > 0 else None,
        "expectation_passes_executed": cnt2["contraction_passes"] - cnt["contraction_passes"],
        "expectation_contraction_calls": cnt2["contraction_calls"] - cnt["contraction_calls"],
        "expectation_bytes_moved_per_rank": cnt2["contraction_bytes"] - cnt["contraction_bytes"],
        "expectation_GBs_per_gpu": (cnt2["contraction_bytes"] - cnt["contraction_bytes"]) / t_exp / 1e9,
        "expectation_x_groups_equivalent_GBs_aggregate": 16.0 * 2 ** n * groups / t_exp / 1e9,
        "energy": e, "norm2": n2, "h_norm1": float(np.abs(hc).sum()),
        # this rank's kernel seconds by phase (every section synchronised; ranks sharing one device take it in turn)
        "expectation_local_s": st2["expectation_local_s"], "expectation_remote_compute_s": st2["expectation_remote_s"],
        "expectation_plan": info, "expectation_partners_read": st2["partners_per_read"],
        "exchange_count": st["swaps"], "exchange_bytes_per_rank": swap_bytes, "shard_read_bytes_sent_per_rank": read_bytes,
    }
    # the same rank on eight GPUs with xGMI links (153 GB/s each way): a half-shard exchange crosses ONE link; the partner reads of <H>
    # use one link per partner at once and overlap with the contraction of the previous chunk
    nread = max(1, st2["partners_per_read"])
    out["projected_with_xgmi"] = {
        "rotations_s": t_local + st["swap_s"] * (1.0 if dry_rank is not None else 0.0) + swap_bytes / link,
        "expectation_s": st2["expectation_local_s"] + max(st2["expectation_remote_s"], (read_bytes / nread) / link if read_bytes else 0.0),
        "assumes": "exchange = bytes / 153 GB/s on one link (+ the measured pack / unpack copies of a dry rank); partner reads: one link "
                   "per partner concurrently, hidden behind the contraction when shorter",
    }
    if dry_rank is not None:
        out["dry_rank"] = {"world": world, "rank": rank, "note": "one rank of the job alone on one GPU: own chunks stand in for the partners', "
                           "every kernel, copy and byte count is that rank's; energy and norm are meaningless here"}
        out.pop("energy_check", None)
    out["amplitude_bytes"] = 8 if real_state else 16
    if real_state:
        out["real_storage_through_the_leg"] = bool(sv._storage_real())
    known = SHARDED_KNOWN.get((n, rotations, terms))
    if known is not None and dry_rank is None and not real_state:
        tol = 1e-11 * out["h_norm1"]
        out["energy_check"] = {"expected": known, "abs_diff": abs(e - known), "tol": tol, "ok": bool(abs(e - known) <= tol)}
    del sv
    torch.cuda.empty_cache()
    return out


def sharded_block(args, local_rank, world, rank, barrier):
    """the `sharded` object of the JSON line: configs[4]'s weak curve (n = base + log2 N: the shard keeps its size) and
    strong curve (n = base) through the same code; at N = 1 both are the one-shard run"""
    g = world.bit_length() - 1
    if (1 << g) != world:
        return {"skipped": f"index-bit partition needs a power-of-two world size, got {world}"}
    base = args.sharded_qubits
    block = {"qubits_per_gpu_weak": base, "qubits_strong": base, "seed": SHARDED_SEED,
             "xgmi_link_peak_GBs": XGMI_LINK_GBS,
             "note": "energy of the strong run must not depend on the number of GPUs (same synthetic state and operators)"}
    block["weak"] = sharded_leg(base + g, local_rank, world, rank, args.sharded_rotations, args.sharded_terms, barrier)
    if g and base - g >= 6:
        block["strong"] = sharded_leg(base, local_rank, world, rank, args.sharded_rotations, args.sharded_terms, barrier)
    else:
        block["strong"] = block["weak"]
    if world == 1 and not args.no_scale_proxy:
        # the same leg on a REAL state (float64 shard: the real-amplitude sweeps and <H> kernels)
        block["real_state"] = sharded_leg(base, local_rank, 1, 0, args.sharded_rotations, args.sharded_terms, None, real_state=True)
        # configs[4] at FULL size without eight GPUs: rank 0 of an 8-rank register of base + 3 qubits as a dry rank on this GPU (its
        # shard is the 2^base amplitudes of the weak curve) — that rank's kernels, pack / unpack copies and link bytes, projected on
        # 153-GB/s links.  Rank 0 contracts four partner shards (the most any rank does under the Hermitian halving).
        block["scale_proxy"] = sharded_leg(base + 3, local_rank, 1, 0, args.sharded_rotations, args.sharded_terms, None, dry_rank=(8, 0))
    checks = [(leg, block[leg]["energy_check"]) for leg in ("strong", "weak") if "energy_check" in block[leg]]
    if not checks:
        block["energy_check"] = "no value on record for these sizes"
    elif all(c["ok"] for _, c in checks):
        block["energy_check"] = "ok (" + ", ".join(f"{leg} {block[leg]['n_qubits']} q" for leg, _ in checks) + ")"
    else:
        block["energy_check"] = "MISMATCH " + "; ".join(f"{leg}: |dE| = {c['abs_diff']:.2e} > {c['tol']:.1e}" for leg, c in checks if not c["ok"])
    return block


def mirror_leg():
    """what a caller of the reference's entry points gets (Route B): H2O/STO-3G UCCSD through
    openvqe_amd.ucc_family.get_energy_ucc.EnergyUCC — `ucc_action` one evaluation per call, and the whole `get_energies`
    (two BFGS runs at tol 1e-4, ref:openvqe/ucc_family/get_energy_ucc.py:92-206) with the reference's default jac=None,
    with the opt-in batched forward-difference Jacobian and with the opt-in exact Jacobian"""
    import contextlib
    import io
    from openvqe_amd import chem
    from openvqe_amd.ucc_family.get_energy_ucc import EnergyUCC
    mol = chem.molecule("H2O")
    mol.rhf()
    prob = mol.problem(active=False)
    ham = prob.jw_hamiltonian()
    size, _, spin_ops, theta_mp2, hf = prob.uccsd()
    e_fci = mol.ci_ground_state()[0]
    out = {"workload": f"H2O/STO-3G UCCSD, {size} cluster operators (reference operator order), MP2 guess", "E_FCI": e_fci}
    ucc = EnergyUCC()
    th = np.array(theta_mp2)
    energies = []
    ucc.ucc_action(th, ham, spin_ops, hf, energies)
    reps = 300
    t0 = time.perf_counter()
    for k in range(reps):
        ucc.ucc_action(th + 1e-3 * k, ham, spin_ops, hf, energies)
    dt = (time.perf_counter() - t0) / reps
    out["ucc_action"] = {"us_per_call": 1e6 * dt, "evals_per_s": 1.0 / dt, "energy_at_theta_mp2": float(energies[0])}
    for label, flags in (("default_fd_jacobian_by_scipy", {}), ("batched_gradient", {"batched_gradient": True}),
                         ("adjoint_gradient", {"adjoint_gradient": True})):
        u = EnergyUCC()
        for k, v in flags.items():
            setattr(u, k, v)
        sink = io.StringIO()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(sink):
            it, res = u.get_energies(ham, spin_ops, spin_ops, hf, list(theta_mp2), [0.0] * size, e_fci)
        out["get_energies_" + label] = {"wall_s": time.perf_counter() - t0, "evaluations": len(res["energies_1"]) + len(res["energies_2"]),
                                        "E1": float(it["minimum_energy_result1_guess"][0]),
                                        "E2": float(it["minimum_energy_result2_guess"][0]),
                                        "E1_minus_FCI": float(res["energies1_substracted_from_FCI"])}
    return out


def newest_profile(dir_glob, name):
    """the newest committed `profiles/<dir_glob>/<name>` (round directories sort by name: r2_…, r3_…, …) as a repo-relative path"""
    import glob
    hits = sorted(glob.glob(os.path.join(ROOT, "profiles", dir_glob, name)))
    return os.path.relpath(hits[-1], ROOT) if hits else "(no committed profile)"


def pmc_traffic_per_launch():
    """HBM bytes per launch of the pair-sweep kernel from the newest committed PMC summary (profiles/*/pmc_summary.csv,
    produced by tools/profile_bench.sh with separate --pmc FETCH_SIZE / WRITE_SIZE passes of this same command).
    FETCH_SIZE is doubled as MI355X_MICROARCH.md §HBM prescribes for wide coalesced reads on gfx950; KiB -> bytes."""
    import csv
    import glob
    best = None
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "*", "pmc_summary.csv"))):
        fetch = write = nf = nw = 0.0
        for row in csv.DictReader(open(path)):
            # the 30-qubit sweeps are the non-temporal instances (NTL = true); cached instances belong to the
            # mid-size side workloads of the same run
            if "k_rot_pairs_v<" not in row["kernel"] or ", true, false>" not in row["kernel"]:
                continue
            n = float(row["dispatches"])
            if row["counter"] == "FETCH_SIZE":
                fetch += float(row["mean_KiB"]) * n
                nf += n
            elif row["counter"] == "WRITE_SIZE":
                write += float(row["mean_KiB"]) * n
                nw += n
        if nf and nw:
            best = ((2.0 * fetch / nf + write / nw) * 1024.0, os.path.relpath(path, ROOT))
    return best


def cpu_baseline_leg(ham, gens, hf, thetas, budget_s=12.0):
    """Oracle C restatement timed on the host cores, one evaluation per core at a time (the fastest CPU
    arrangement at 14 qubits): C2 = fused mask sweeps (same algorithm as the HIP kernels), C1 = gate-level
    CNOT-staircase circuit + term-wise observable (what one reference/myQLM evaluation does algorithmically)."""
    from oracle import cref
    from openvqe_amd.backend import compile_ucc_program
    flags = cref.use_native_build() if cref._lib is None else "as loaded"
    n = ham.nbqbits
    rx, rz, rc, pidx, K = compile_ucc_program(n, gens)
    hx, hz, hc = ham.packed()
    hc = hc.real.copy()
    L = cref.lib()
    cores = cref.usable_cpus()
    out = {}
    for mode, label in ((0, "fused"), (1, "gate_level")):
        cref.ucc_energy_batch(n, hf, rx, rz, rc, pidx, thetas[:cores], hx, hz, hc, ham.constant_coeff, mode)  # warm
        t0 = time.perf_counter()
        cnt = 0
        e = None
        while True:
            e = cref.ucc_energy_batch(n, hf, rx, rz, rc, pidx, thetas[:cores], hx, hz, hc, ham.constant_coeff, mode)
            cnt += min(cores, thetas.shape[0])
            dt = time.perf_counter() - t0
            if dt > budget_s / 2:
                break
        out[label] = {"evals_per_s": cnt / dt, "evals": cnt, "seconds": dt, "threads": cores, "energy0": float(e[0]),
                      "energies": np.asarray(e, np.float64).copy()}
    # the fused CPU sweep beside the GPU's single-Pauli-string sweep (26 qubits = 1 GiB, OpenMP over the cores)
    from openvqe_amd.operators import pack_string
    nq = 26
    psi = np.zeros(1 << nq, np.complex128)
    psi[0] = 1.0
    x, z = pack_string(nq, "XXXY", [0, 9, 17, nq - 1])
    L.orc_pauli_rotation(psi, nq, int(x), int(z), 0.1)
    t0 = time.perf_counter()
    reps = 3
    for _ in range(reps):
        L.orc_pauli_rotation(psi, nq, int(x), int(z), 0.1)
    dt = (time.perf_counter() - t0) / reps
    out["sweep_26q"] = {"ms": 1e3 * dt, "GBs": 32.0 * (1 << nq) / dt / 1e9, "threads": cores}
    out["cflags"] = flags
    return out, cores


LINE_LIMIT = 4096   # the driver's parser gave up on a 22-KB line (round 4): the printed line stays below this, tested
POOL_BLOCKS = 32    # distinct B x K parameter blocks resident in HBM; steps beyond this many cycle through them
DUMP_LIMIT_BYTES = 64 << 20   # --dump-outputs: at most this much is written


def _r(v, digits=6):
    """floats of the printed line at `digits` significant digits (the full-precision numbers are in bench_extra.json)"""
    if isinstance(v, float):
        if v != v or v in (float("inf"), float("-inf")):
            return None     # strict JSON: no NaN / Infinity on the line
        return float(f"{v:.{digits}g}")
    return v


def compact_line(out, extra_path):
    """The ONE line the driver parses: the contract's keys, `roofline` (without the per-string rows), `cpu_baseline` and a
    dozen scalar side figures; everything else (side workloads, program_info dumps, the sharded legs' detail) is in
    `bench_extra.json`, whose path the line names."""
    keep = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data", "config")
    line = {k: out[k] for k in keep if k in out}
    line["data"] = "synthetic theta ~ U(-0.1, 0.1); H2O/STO-3G Hamiltonian + UCCSD generators computed in-repo"
    if "roofline" in out:
        rf = out["roofline"]
        line["roofline"] = {k: _r(rf.get(k)) for k in ("bound", "achieved", "peak", "unit", "frac", "traffic")}
        line["roofline"].update(kernel="k_rot_pairs_v", workload=f"single-Pauli-string sweep, {rf.get('qubits')} qubits",
                                avg_launch_ms=_r(rf.get("avg_launch_ms")), bytes_per_launch=rf.get("bytes_per_launch"),
                                traffic_source=rf.get("traffic_source"))
    if "cpu_baseline" in out:
        cb = out["cpu_baseline"]
        line["cpu_baseline"] = {k: _r(cb.get(k)) for k in ("value", "unit", "cores", "kind", "sample",
                                                           "gate_level_evals_per_s", "gpu_minus_cpu_energy",
                                                           "batch_kernel_max_abs_diff_vs_oracle")}
    side = {}
    for k in ("single_call_evals_per_s", "fd_gradient_evals_per_s", "mirror_ucc_action_evals_per_s"):
        if k in out:
            side[k] = _r(out[k])
    s24 = out.get("summary_24_qubits") or {}
    for k_out, k_in in (("uccsd24_evaluation_ms", "uccsd_evaluation_ms"), ("uccsd24_gradient_ms", "uccsd_gradient_1715_parameters_ms"),
                        ("n2_quccsd_evaluation_ms", "n2_quccsd_evaluation_ms"), ("n2_quccsd_gradient_ms", "n2_quccsd_gradient_ms")):
        if s24.get(k_in) is not None:
            side[k_out] = _r(s24[k_in])
    if "setup_ms" in s24:
        side["setup_ms_n2_uccsd"] = _r(s24["setup_ms"].get("n2_uccsd"))
        side["setup_ms_n2_quccsd"] = _r(s24["setup_ms"].get("n2_quccsd"))
    if side:
        line["side"] = side
    sh = out.get("sharded")
    if sh is not None:
        if "error" in sh or "skipped" in sh:
            line["sharded"] = {k: str(sh[k])[:300] for k in ("error", "skipped") if k in sh}
        else:
            line["sharded"] = {
                "weak_qubits": sh["weak"]["n_qubits"], "strong_qubits": sh["strong"]["n_qubits"],
                "weak_energy": sh["weak"]["energy"], "strong_energy": sh["strong"]["energy"],
                "weak_rotations_s": _r(sh["weak"]["rotations_s"]), "weak_expectation_s": _r(sh["weak"]["expectation_s"]),
                "strong_rotations_s": _r(sh["strong"]["rotations_s"]), "strong_expectation_s": _r(sh["strong"]["expectation_s"]),
                "energy_check": sh.get("energy_check")}
            for leg in ("weak", "strong"):
                line["sharded"][leg + "_compute_s"] = [_r(sh[leg].get(k), 4) for k in ("local_sweeps_s", "expectation_local_s", "expectation_remote_compute_s")]
            if sh.get("real_state"):
                line["sharded"]["real_state_rotations_s"] = _r(sh["real_state"]["rotations_s"], 4)
                line["sharded"]["real_state_expectation_s"] = _r(sh["real_state"]["expectation_s"], 4)
            px = sh.get("scale_proxy")
            if px is not None:
                line["sharded"]["scale_proxy"] = {
                    "what": "rank 0 of 8 at %d qubits, alone on this GPU (dry rank)" % px["n_qubits"],
                    "local_sweeps_s": _r(px["local_sweeps_s"], 4), "expectation_local_s": _r(px["expectation_local_s"], 4),
                    "expectation_remote_compute_s": _r(px["expectation_remote_compute_s"], 4),
                    "exchanges": px["exchange_count"], "exchanged_GiB": _r(px["exchanged_GiB_per_rank"], 4),
                    "shard_read_GiB": _r(px["shard_read_GiB_per_rank"], 4), "partners_read": px["expectation_partners_read"],
                    "projected_8gpu_rotations_s": _r(px["projected_with_xgmi"]["rotations_s"], 4),
                    "projected_8gpu_expectation_s": _r(px["projected_with_xgmi"]["expectation_s"], 4)}
    line["extra"] = extra_path
    return line


def emit(out):
    """write the full record to bench_extra.json (gpurun_out/ when it exists, so that it travels back from a GPU box), then
    print the compact line LAST.  -> the printed text"""
    extra_path = None
    for d in (os.path.join(ROOT, "gpurun_out"), ROOT, "/tmp"):
        if os.path.isdir(d) and os.access(d, os.W_OK):
            try:
                path = os.path.join(d, "bench_extra.json")
                with open(path, "w") as f:
                    json.dump(out, f, indent=1)
                extra_path = os.path.relpath(path, ROOT) if d != "/tmp" else path
                break
            except OSError:
                continue
    text = json.dumps(compact_line(out, extra_path), allow_nan=False)
    assert len(text) < LINE_LIMIT, f"bench line is {len(text)} bytes (limit {LINE_LIMIT})"
    # RCCL / gloo write their banners to the C-level stdout buffer; drain it so that the JSON line is the LAST line
    import ctypes
    try:
        ctypes.CDLL(None).fflush(None)
    except OSError:
        pass
    sys.stdout.flush()
    print(text, flush=True)
    return text


def launch_ranks(n_gpus):
    """`python bench.py --gpus N` without a launcher: start `python -m torch.distributed.run --nproc-per-node N bench.py
    <same arguments>` as a child process on a free local port, pass its stdout through line by line and print the JSON
    line of rank 0 LAST (whatever a rank or RCCL wrote after it).  -> the child's exit code."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC: what RCCL needs between the ranks on this driver
    from openvqe_amd.common_files.host_threads import usable_cpus   # (no GPU call: the parent must not touch the device)
    env.setdefault("OMP_NUM_THREADS", str(max(1, usable_cpus() // n_gpus)))   # the container's CPU quota shared between the ranks
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n_gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    child = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, text=True, bufsize=1)
    line_json = None
    for ln in child.stdout:
        if ln.startswith("{") and '"metric"' in ln:
            line_json = ln.rstrip("\n")      # held back: printed after everything else
            continue
        sys.stdout.write(ln)
        sys.stdout.flush()
    rc = child.wait()
    if line_json is not None:
        assert len(line_json) < LINE_LIMIT, f"bench line is {len(line_json)} bytes (limit {LINE_LIMIT})"
        print(line_json, flush=True)
    return rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=65536, help="parameter vectors per step per GPU")
    ap.add_argument("--roofline-qubits", type=int, default=30)
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-extra", action="store_true", help="skip the H2 / LiH / H2O latency and small-batch side figures")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--no-sharded", action="store_true", help="skip the index-bit-partitioned configs[4] block")
    ap.add_argument("--sharded-qubits", type=int, default=int(os.environ.get("OVQE_BENCH_SHARDED_QUBITS", "31")),
                    help="configs[4]: qubits per GPU of the weak curve = register of the strong curve (31: 32-GiB shards)")
    ap.add_argument("--no-scale-proxy", action="store_true", help="skip the dry 8-rank leg of configs[4] (one rank of 34 qubits on this GPU)")
    ap.add_argument("--sharded-rotations", type=int, default=64)
    ap.add_argument("--sharded-terms", type=int, default=1000)
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also run the side legs: dense-kernel cross-check, sharded block, HBM roofline "
                         "sweeps, side workloads, CPU baseline (each still subject to its --no-* flag); off: the headline figure only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the energies of the last timed step (rank 0) to DIR/energies.npy (float64)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # plain `python bench.py --gpus N`: this process has not touched the GPU and never will — it starts the N ranks
        # as a fresh child (never exec), relays their output and leaves with their exit code
        sys.exit(launch_ranks(args.gpus))

    import torch

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    backend = os.environ.get("OVQE_BENCH_BACKEND", "nccl")  # "gloo": functional test of the N>1 path on one GPU
    if os.environ.get("OVQE_BENCH_SINGLE_DEVICE"):
        local_rank = 0
    use_dist = world > 1 or bool(os.environ.get("OVQE_BENCH_FORCE_DIST"))  # force: exercise the RCCL path at N=1
    if use_dist:
        import torch.distributed as dist
        torch.cuda.set_device(local_rank)
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend)
    if world != args.gpus:
        sys.exit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: start one rank per GPU (plain `python bench.py --gpus N` "
                 "does it by itself, or `python -m torch.distributed.run --nproc-per-node N bench.py --gpus N`)")

    import __graft_entry__ as entry
    if use_dist:
        # one builder per node (the .so is shared in-tree); the others wait for it
        if local_rank == 0:
            entry.build()
        dist.barrier()
    else:
        entry.build()
    from openvqe_amd.backend import Statevector

    ham, gens, hf = build_workload()
    n = ham.nbqbits
    K = len(gens)
    R = sum(len(g.terms) for g in gens)
    G = len(set(ham.packed()[0].tolist()))
    B = args.batch
    rng = np.random.default_rng(140 + rank)
    # inputs resident in HBM before the timed region: every step reads a B x K parameter block from device memory and
    # leaves B energies there; the energies of each step are copied back to the host inside the step.  Step k (warm-up
    # steps first) uses block k % nblocks: up to POOL_BLOCKS steps every step has its own block, beyond that they cycle,
    # so that memory does not grow with --steps (one block is B * K * 8 bytes: 73 MB at the defaults).
    nblocks = min(args.steps + args.warmup, POOL_BLOCKS)
    dev = torch.device("cuda", local_rank)
    thetas_host = rng.uniform(-0.1, 0.1, size=(nblocks, B, K))
    thetas_dev = torch.from_numpy(thetas_host).to(dev)
    energies_dev = torch.empty((nblocks, B), dtype=torch.float64, device=dev)

    sv = Statevector(n, device=local_rank)
    sv.set_hamiltonian(ham)
    sv.set_ucc_program(gens, hf)

    def sync_all():
        torch.cuda.synchronize()
        if use_dist:
            dist.barrier()
            torch.cuda.synchronize()

    host_energies = torch.empty((B,), dtype=torch.float64).pin_memory()   # where the optimiser reads them: no staging copy

    def step(k):
        k %= nblocks
        sv.energy_batch_device(B, thetas_dev[k].data_ptr(), energies_dev[k].data_ptr())
        host_energies.copy_(energies_dev[k])   # blocking device-to-host copy: the step ends with the energies on the host
        return host_energies

    def timed_steps(first, count):
        sync_all()
        t0 = time.perf_counter()
        kms = 0.0
        last = None
        for k in range(first, first + count):
            last = step(k)
            kms += sv.last_batch_ms()
        sync_all()
        return time.perf_counter() - t0, kms, last

    for w in range(args.warmup):
        step(w)
    elapsed, kernel_ms, e = timed_steps(args.warmup, args.steps)
    if use_dist:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cuda" if backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    total_evals = world * B * args.steps
    value = total_evals / elapsed
    e = e.numpy().copy()
    if rank == 0 and args.dump_outputs:
        # what a caller of the timed path receives from the last timed step: its B energies (float64, B * 8 bytes; above
        # DUMP_LIMIT_BYTES a fixed, seeded sample of them in index order)
        os.makedirs(args.dump_outputs, exist_ok=True)
        dump = e.astype(np.float64)
        if dump.nbytes > DUMP_LIMIT_BYTES:
            keep = DUMP_LIMIT_BYTES // dump.itemsize
            dump = dump[np.sort(np.random.default_rng(0).choice(dump.size, keep, replace=False))]
        np.save(os.path.join(args.dump_outputs, "energies.npy"), dump)

    # the same steps on the dense LDS statevector kernel (support compaction off), rank 0, for the record
    dense = None
    if rank == 0 and args.full:
        sv.set_option("force_path", 1)
        nd = max(1, min(args.steps, 3))
        bd = min(B, 8192)
        slots = [(args.warmup + k) % nblocks for k in range(nd)]
        dense_out = torch.empty((nd, bd), dtype=torch.float64, device=dev)
        t0 = time.perf_counter()
        kd = 0.0
        for k in range(nd):
            sv.energy_batch_device(bd, thetas_dev[slots[k]].data_ptr(), dense_out[k].data_ptr())
            kd += sv.last_batch_ms()
        torch.cuda.synchronize()
        dense = {"evals_per_s": nd * bd / (time.perf_counter() - t0), "kernel_only_evals_per_s": nd * bd / (kd * 1e-3),
                 "batch": bd, "max_abs_diff_vs_value_path": float(
                     (dense_out - energies_dev[slots, :bd]).abs().max().item())}
        sv.set_option("force_path", 0)

    out = {
        "metric": "vqe_energy_evals_per_sec",
        "value": value,
        "unit": "evals/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": 1e3 * elapsed / args.steps,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f64",
        "data": "synthetic parameter vectors theta ~ U(-0.1, 0.1); H2O/STO-3G Hamiltonian and UCCSD generators "
                "computed in-repo from first principles (no dataset / checkpoint involved)",
        "config": {
            "workload": "H2O/STO-3G UCCSD energy evaluation (the metric's config): 14 qubits, "
                        f"{K} generators = {R} Pauli rotations, JW Hamiltonian {len(ham.terms) + 1} terms / {G} x-groups",
            "batch_per_gpu": B,
            "parallelism": f"batch-replicas x{world}",
        },
    }
    # configs[4]: the index-bit-partitioned register through the same launch (every rank takes part; outside the timed steps).
    # Every collective wait of it sits under a deadline (openvqe_amd.distributed.DistWatchdog, OVQE_DIST_TIMEOUT_S, default 120 s
    # without progress): on expiry rank 0 prints the line with "sharded": {"error": ...} and every rank leaves with exit code 3
    if args.full and not args.no_sharded:
        from openvqe_amd import distributed as _dd

        def expired(phase, seconds):
            if rank == 0:
                out["sharded"] = {"error": f"rank 0: no progress for {seconds:.0f} s in '{phase}' (OVQE_DIST_TIMEOUT_S); "
                                           f"world size {world}, backend {backend if use_dist else 'none'}"}
                emit(out)
            sys.stdout.flush()
            sys.stderr.write(f"bench.py rank {rank}: sharded leg made no progress for {seconds:.0f} s in '{phase}'; leaving\n")
            sys.stderr.flush()
            if rank != 0:
                # the launcher ends every rank as soon as one has left: rank 0 (whose deadline started at ITS last progress, later
                # than a stalled rank's) gets one more period to print the line before this rank's exit takes it down
                time.sleep(_dd.watchdog.timeout_s if _dd.watchdog is not None else 10.0)

        if use_dist:
            _dd.watchdog = _dd.DistWatchdog(on_expire=expired)
        sharded_error = None
        try:
            out["sharded"] = sharded_block(args, local_rank, world, rank, dist.barrier if use_dist else None)
        except Exception as exc:   # the replica figures above are measured: the line carries them, and what went wrong here
            sharded_error = f"rank {rank}: {type(exc).__name__}: {exc}"[:400]
            out["sharded"] = {"error": sharded_error}
            sys.stderr.write(f"bench.py rank {rank}: sharded leg failed: {sharded_error}\n")
        finally:
            if _dd.watchdog is not None:
                _dd.watchdog.stop()
                _dd.watchdog = None
        if sharded_error is not None and use_dist:
            # several ranks and a failed collective path: the ranks are no longer in step (and the process group may be unusable) — no
            # further barrier; rank 0 prints the line, every rank leaves with the exit code of the watchdog's way out
            if rank == 0:
                emit(out)
            sys.stdout.flush()
            sys.stderr.flush()
            os._exit(3)
    if rank == 0:
        e_last = float(e[0])
        # kernel-only figures of the timed region (HIP events around the fused launch)
        per_eval_bytes = 32.0 * (1 << n) * R + 16.0 * (1 << n) * G
        out["timed_kernel"] = {
            "name": "k_sparse_vqe_rows (support-compacted evaluation: the circuit's reachable support is 441 of 16384 "
                    "amplitudes; exact, see DESIGN.md; flat rows of padded 64-bit pair words) — auto-selected by ovqe_energy_batch",
            "avg_launch_ms": kernel_ms / args.steps,
            "evals_per_s_kernel_only": B * args.steps / (kernel_ms * 1e-3),
            "algorithmic_GBs_if_streamed": per_eval_bytes * B * args.steps / (kernel_ms * 1e-3) / 1e9,
            "note": "state is LDS-resident by design; this is not HBM traffic",
            "sample_energy": e_last,
            "dense_lds_statevector_kernel": dense,
        }
        # the kernel behind `value` keeps its states in LDS: its roofline is the LDS array, not HBM.  Bytes per
        # evaluation from the compiled program: an active pair = 2 reads + 2 writes of 8-B amplitudes + one 16-B cos/sin
        # entry (its 8-B word streams from L2); a Hamiltonian entry = 2 amplitude reads (the 16-B entry record streams from L2).
        info = sv.program_info()
        lds_bytes = 48.0 * info["sp_pairs"] + 16.0 * info["sp_h_entries"]
        lds_rate = lds_bytes * B * args.steps / (kernel_ms * 1e-3) / 1e9
        out["roofline_value_kernel"] = {
            "bound": "lds", "kernel": "k_sparse_vqe_rows<2>", "achieved": lds_rate, "peak": LDS_PEAK_GBS, "unit": "GB/s",
            "frac": lds_rate / LDS_PEAK_GBS, "lds_bytes_per_evaluation": lds_bytes,
            "active_pairs_per_evaluation": info["sp_pairs"], "hamiltonian_entries_per_evaluation": info["sp_h_entries"],
            "support": info["support"], "avg_launch_ms": kernel_ms / args.steps,
            "note": "aggregate LDS read rate of MI355X_MICROARCH.md (ds_read_b64/b128, every CU streaming); the kernel is NOT "
                    "bound by the LDS array (rocprofv3 counters, profiles/r3a: LDS instructions active 6 % of the wave cycles, "
                    "bank-conflict cycles cut by a third without any change in run time) but by instruction issue and the "
                    "latency of the dependent chain amplitudes -> rotate -> store of consecutive rows on one wave",
        }
        if args.full and not args.no_roofline:
            sv.close()
            nq = args.roofline_qubits
            rows = roofline_leg(local_rank, nq)
            pair_rows = [r for r in rows if not r["diag"]]
            worst = min(pair_rows, key=lambda r: r["GBs"])
            mean_ms = float(np.mean([r["ms"] for r in pair_rows]))
            achieved = 32.0 * (1 << nq) / (mean_ms * 1e-3) / 1e9
            out["roofline"] = {
                "bound": "hbm",
                "kernel": "k_rot_pairs_v<64|128,1,nt> (single-Pauli-string sweep, in place, one pair per thread)",
                "workload": f"exp(-i 0.1 P) on a {nq}-qubit random state, {len(pair_rows)} strings (SURVEY §8d M1), "
                            "mean over strings of the HIP-event average of 20 launches",
                "achieved": achieved,
                "peak": HBM_PEAK_GBS,
                "unit": "GB/s",
                "frac": achieved / HBM_PEAK_GBS,
                # PMC counters need their own rocprofv3 passes (no counters inside this run): the number below is read from the
                # newest COMMITTED profile of this same command and says so
                "traffic": (pmc_traffic_per_launch() or (None, None))[0] if nq == 30 else None,
                "traffic_source": ("committed profile: " + pmc_traffic_per_launch()[1]) if nq == 30 and pmc_traffic_per_launch() else None,
                "bytes_per_launch": 32 * (1 << nq),
                "qubits": nq,
                "avg_launch_ms": mean_ms,
                "worst_string": worst,
                "per_string": rows,
            }
        if args.full and not args.no_extra and world == 1:  # side figures belong to the single-GPU line; N > 1 ranks only wait
            out["extra_workloads"] = extra_workloads_leg(local_rank)
            # what the reference's callers see on this workload (H2O/STO-3G UCCSD), lifted out of the side figures:
            # `value` is the resident-batch throughput; scipy's optimisers call ONE evaluation at a time
            # (ref:openvqe/ucc_family/get_energy_ucc.py:158-175), the opt-in batched forward-difference gradient is K + 1
            # evaluations per call, and host-side parameter buffers add the PCIe upload
            h2o = next(r for r in out["extra_workloads"] if r.get("molecule") == "H2O")
            out["single_call_evals_per_s"] = h2o["single"]["evals_per_s"]
            out["fd_gradient_evals_per_s"] = h2o["fd_gradient"]["evals_per_s"]
            out["host_buffer_evals_per_s"] = h2o["batch4096"]["evals_per_s"]
            # ... and through the mirrors of the reference's entry points (what north_star names)
            mir = mirror_leg()
            out["mirror"] = mir
            out["mirror_ucc_action_evals_per_s"] = mir["ucc_action"]["evals_per_s"]
            out["mirror_get_energies_wall_s"] = {k[len("get_energies_"):]: v["wall_s"] for k, v in mir.items() if k.startswith("get_energies_")}
            # ... and the 24-qubit figures (BASELINE configs[3] on its molecule), lifted out the same way
            m3 = next((r for r in out["extra_workloads"] if "M3" in r.get("workload", "")), None)
            n2 = next((r for r in out["extra_workloads"] if "configs[3]" in r.get("workload", "")), None)
            if m3 and n2:
                out["summary_24_qubits"] = {
                    "uccsd_evaluation_ms": m3["sector_path"]["ms_steady_state"],
                    "uccsd_evaluation_ms_in_batches_of_64": m3["sector_path"]["batch_64"]["ms_per_evaluation"],
                    "uccsd_evaluation_hamiltonian_kernel": {k: m3["sector_path"]["roofline_expect_kernel"][k]
                                                            for k in ("bound", "achieved", "peak", "unit", "frac", "avg_launch_ms")},
                    "uccsd_evaluation_circuit_sweeps_ms": m3["sector_path"]["circuit_sweeps_ms"],
                    "uccsd_evaluation_ms_dense_state": m3["dense_state_compact_cover"]["ms_steady_state"],
                    "uccsd_gradient_1715_parameters_ms": m3["sector_path"]["ms_gradient_all_parameters"],
                    "uccsd_gradient_ms_dense_state": m3["dense_state_compact_cover"]["ms_gradient_all_parameters"],
                    "n2_uccsd_vqe": {k: n2["uccsd_vqe_lbfgs_exact_gradient"][k] for k in ("energy", "iterations", "gradient_calls", "wall_s")},
                    "n2_quccsd_vqe": {k: n2["quccsd_vqe_lbfgs_exact_gradient"][k] for k in ("energy", "iterations", "gradient_calls", "wall_s")},
                    "n2_quccsd_evaluation_ms": n2["quccsd_gate_list_at_theta_mp2"]["ms_steady_state"],
                    "n2_quccsd_gradient_ms": n2["quccsd_vqe_lbfgs_exact_gradient"]["ms_per_gradient_call_steady"],
                    "roofline_quccsd24": n2.get("roofline_quccsd24"),
                    "setup_ms": {"n2_uccsd": n2["uccsd_at_theta_mp2"]["setup_ms"]["total"],
                                 "n2_quccsd": n2["quccsd_gate_list_at_theta_mp2"]["setup_ms"]["total"]},
                    "n2_uccsd_vqe_wall_s_including_setup": n2["uccsd_vqe_lbfgs_exact_gradient"]["wall_s"]
                                                           + 1e-3 * n2["uccsd_at_theta_mp2"]["setup_ms"]["total"],
                    "n2_fci_627264_determinants": {k: n2["fci_of_the_sector_lanczos"][k] for k in ("energy", "iterations", "wall_s")},
                    "n2_fermionic_adapt_30_iterations": n2.get("fermionic_adapt_30_iterations"),
                }
        if args.full and not args.no_cpu and world == 1:
            # the oracle evaluates the first `cores` parameter vectors of the FIRST TIMED step; the energies the timed launch
            # (k_sparse_vqe_rows, B-wide) left in HBM for those vectors are compared with them: the kernel behind `value` is
            # checked in the run that times it (the single-call kernel keeps its own check beside it)
            kt = args.warmup
            kb = kt % nblocks   # its parameter block (and energy slot, last written by a timed step on the same block)
            cpu, cores = cpu_baseline_leg(ham, gens, hf, thetas_host[kb], args.cpu_seconds)
            e_gpu0 = energy_check(ham, gens, hf, thetas_host[kb, 0], local_rank)
            nchk = min(cores, B)
            e_timed = energies_dev[kb, :nchk].cpu().numpy()
            batch_diff = {lab: float(np.abs(e_timed - cpu[lab].pop("energies")[:nchk]).max()) for lab in ("fused", "gate_level")}
            out["cpu_baseline"] = {
                "value": cpu["fused"]["evals_per_s"],
                "unit": "evals/s",
                "cores": cores,
                "kind": "port",
                "sample": f"{cpu['fused']['evals']} evaluations of the same 14-qubit workload in "
                          f"{cpu['fused']['seconds']:.1f} s with oracle/c fused sweeps, one evaluation per core "
                          f"(OpenMP x{cores}); the gate-level restatement of the reference's myQLM algorithm "
                          f"(CNOT staircase gate by gate, observable term by term) on the same cores: "
                          f"{cpu['gate_level']['evals_per_s']:.2f} evals/s over {cpu['gate_level']['evals']} evaluations",
                "cflags": cpu["cflags"],
                "gate_level_evals_per_s": cpu["gate_level"]["evals_per_s"],
                "single_string_sweep_26_qubits": cpu["sweep_26q"],
                "gpu_minus_cpu_energy": e_gpu0 - cpu["fused"]["energy0"],
                "batch_kernel_max_abs_diff_vs_oracle": batch_diff["fused"],
                "batch_kernel_max_abs_diff_vs_gate_level_oracle": batch_diff["gate_level"],
                "batch_kernel_checked": f"energies of the timed step {kt} (launch of {B}), first {nchk} parameter vectors",
            }
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        emit(out)


def energy_check(ham, gens, hf, theta, device):
    from openvqe_amd.backend import Statevector
    with Statevector(ham.nbqbits, device=device) as sv:
        sv.set_hamiltonian(ham)
        sv.set_ucc_program(gens, hf)
        return sv.energy(theta)


if __name__ == "__main__":
    main()
