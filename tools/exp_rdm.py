"""Two-particle density matrix of a UCCSD state: ovqe_rdm (Statevector.rdm2) against the route that existed before it — the upper
triangle of D2 as one CSR operator per element through Statevector.bilinear_batch — in the same process on the same state.
  cases: h2o = H2O/STO-3G UCCSD, 14 qubits, random angles;  n2 = N2/cc-pVDZ (10e,12o) UCCSD at the MP2 amplitudes, 24 qubits
  python tools/exp_rdm.py [--out DIR] [--reps N] [--base-reps N] [case ...]     every case in a child process under its own `timeout`
  python tools/exp_rdm.py --case NAME [...]                                       one case, in this process
Times: wall clock around synchronous calls (both routes return with the result on the host), median after a warm-up; the split of
rdm2 by kernel from the HIP events of ovqe_rdm_info.  One JSON line per case (and DIR/rdm_<case>.json)."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIMITS = {"h2o": 240, "n2": 900}   # seconds per child


def _arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def build_case(name):
    import numpy as np
    from openvqe_amd import chem, fermion
    if name == "h2o":
        mol = chem.molecule("H2O")
        mol.rhf()
        ham, gens, hf = mol.jw_hamiltonian(), fermion.uccsd_generators(mol.nao, mol.n_elec // 2), mol.hf_init()
        theta = np.random.default_rng(2).uniform(-0.2, 0.2, len(gens))
        hpq, hpqrs = fermion.spin_orbital_integrals(mol.h_mo, mol.eri_mo)
        return ham, gens, hf, theta, hpq, hpqrs, mol.nuclear_repulsion()
    if name == "n2":
        mol = chem.molecule("N2-CCPVDZ")
        mol.rhf()
        prob = chem.cas_problem(mol, 2, 12)
        _, _, spin_ops, theta_mp2, hf = prob.uccsd()
        return prob.jw_hamiltonian(), spin_ops, hf, np.array(theta_mp2), prob.hpq, prob.hpqrs, prob.constant
    raise SystemExit(f"unknown case {name}")


def d2_upper_operators(n):
    """CSR Pauli sums (index-bit masks) of a+_p a+_q a_s a_r for the pair indices i <= j, in row-major order of the upper triangle"""
    import numpy as np
    from openvqe_amd import fermion
    pairs = [(p, q) for p in range(n) for q in range(p + 1, n)]
    cc = [fermion.jw_product([(p, True), (q, True)]) for p, q in pairs]
    aa = [fermion.jw_product([(s, False), (r, False)]) for r, s in pairs]
    offsets, xs, zs, cs = [0], [], [], []
    for i in range(len(pairs)):
        for j in range(i, len(pairs)):
            for (x, z), c in fermion.psum_mul(cc[i], aa[j]).items():
                if c != 0:
                    xs.append(x)
                    zs.append(z)
                    cs.append(c)
            offsets.append(len(xs))
    xs, zs = np.array(xs, np.uint64), np.array(zs, np.uint64)

    def to_index_bits(m):   # jw_product numbers bit q = qubit q; the register has qubit q at bit n-1-q
        out = np.zeros_like(m)
        for q in range(n):
            out |= ((m >> np.uint64(q)) & np.uint64(1)) << np.uint64(n - 1 - q)
        return out
    return np.array(offsets, np.int64), to_index_bits(xs), to_index_bits(zs), np.array(cs, np.complex128)


def run_case(name, reps, base_reps, out_dir):
    import numpy as np
    from openvqe_amd import rdm
    from openvqe_amd.backend import Statevector
    ham, gens, hf, theta, hpq, hpqrs, constant = build_case(name)
    n = ham.nbqbits
    P = n * (n - 1) // 2
    t0 = time.perf_counter()
    offsets, xs, zs, cs = d2_upper_operators(n)
    t_ops = time.perf_counter() - t0
    res = {"case": name, "qubits": n, "pairs": P, "baseline_operators": len(offsets) - 1, "baseline_strings": int(len(xs)),
           "baseline_distinct_x": int(len(np.unique(xs))), "baseline_operator_build_s": round(t_ops, 2)}
    with Statevector(n) as sv:
        sv.set_hamiltonian(ham)
        sv.set_ucc_program(gens, hf)
        e_h = sv.energy(theta)
        sv.prepare_state(theta)
        print(f"[{name}] state prepared", file=sys.stderr, flush=True)
        d2 = sv.rdm2(packed=True)                       # warm-up: buffers, code objects
        times, split = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            d2 = sv.rdm2(packed=True)
            times.append(time.perf_counter() - t0)
            split.append(sv.rdm_info())
        info = split[-1]
        res.update({"rdm2_ms_median": 1e3 * float(np.median(times)), "rdm2_ms_all": [round(1e3 * t, 3) for t in times],
                    "rdm_info": info,
                    "rdm2_split_us_median": {k: float(np.median([s[k] for s in split])) for k in ("list_us", "rows_us", "gram_us", "finish_us")}})
        t1 = []
        for _ in range(reps):
            t0 = time.perf_counter()
            g1 = sv.rdm1()
            t1.append(time.perf_counter() - t0)
        res["rdm1_ms_median"] = 1e3 * float(np.median(t1))
        # the energy re-assembled from the integrals against the Hamiltonian kernels
        e_rdm = rdm.energy(hpq, hpqrs, constant, g1, rdm.unpack_rdm2(d2, n))
        N, sz, s2 = rdm.spin_expectations(g1, rdm.unpack_rdm2(d2, n))
        res.update({"energy_hamiltonian": e_h, "energy_rdm": e_rdm, "N": N, "Sz": sz, "S2": s2})
        # the route of the parent commit, same process, same state
        print(f"[{name}] rdm2 {res['rdm2_ms_median']:.3f} ms; baseline ...", file=sys.stderr, flush=True)
        base = sv.bilinear_batch(offsets, xs, zs, cs)   # warm-up
        tb = []
        for _ in range(base_reps):
            t0 = time.perf_counter()
            base = sv.bilinear_batch(offsets, xs, zs, cs)
            tb.append(time.perf_counter() - t0)
            print(f"[{name}] baseline call {tb[-1]:.3f} s", file=sys.stderr, flush=True)
        iu = np.triu_indices(P)
        res.update({"baseline_ms_median": 1e3 * float(np.median(tb)), "baseline_ms_all": [round(1e3 * t, 3) for t in tb],
                    "max_abs_difference": float(np.abs(base - d2[iu]).max())})
    res["ratio_baseline_over_rdm2"] = res["baseline_ms_median"] / res["rdm2_ms_median"]
    # work by construction (the figures the rates are quoted against)
    rows, wpad = info["rows"], -(-P // 64) * 64
    res["gram_flop"] = (2 if info["real"] else 8) * rows * info["block_pairs"] * 64 * 64
    res["rows_bytes_written"] = rows * wpad * (8 if info["real"] else 16)
    if info["gram_us"] > 0:
        res["gram_tflops"] = res["gram_flop"] / (res["rdm2_split_us_median"]["gram_us"] * 1e-6) / 1e12
    print(json.dumps(res), flush=True)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, f"rdm_{name}.json"), "w") as f:
            json.dump(res, f, indent=1)


def main():
    reps, base_reps, out_dir = _arg("--reps", 7), _arg("--base-reps", 5), _arg("--out", "")
    if "--case" in sys.argv:
        run_case(_arg("--case", ""), reps, base_reps, out_dir)
        return
    skip, cases = False, []
    for a in sys.argv[1:]:
        if skip:
            skip = False
        elif a in ("--reps", "--base-reps", "--out"):
            skip = True
        elif not a.startswith("--"):
            cases.append(a)
    for name in cases or ["h2o", "n2"]:
        cmd = ["timeout", "-k", "10", str(LIMITS[name]), sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(reps),
               "--base-reps", str(base_reps)] + (["--out", out_dir] if out_dir else [])
        rc = subprocess.call(cmd)
        if rc != 0:   # a fault, an abort or a time limit: nothing more is started on the device
            raise SystemExit(f"case {name} ended with status {rc}: stopping")


if __name__ == "__main__":
    main()
