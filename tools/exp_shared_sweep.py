"""batch threshold of the workgroup geometry of the rows form: H2O/STO-3G UCCSD (or mol=LiH, ...) at B = 2048 ... 65536 on both geometries in one
process ("sparse_shared" = 2: k_sparse_vqe_rows_shared at every batch size, 0: k_sparse_vqe_rows<2>), alternating, kernel time by HIP
events.  Needs the testing build (OVQE_LIB=testing).  python tools/exp_shared_sweep.py [geoms=0,2] [reps=9] [mol=H2O]"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from openvqe_amd import chem, fermion
from openvqe_amd.backend import Statevector
args = dict(a.split("=") for a in sys.argv[1:])
geoms = [int(g) for g in args.get("geoms", "0,2").split(",")]
reps = int(args.get("reps", 9))
mol = chem.molecule(args.get("mol", "H2O")); mol.rhf(); ham = mol.jw_hamiltonian(); hf = mol.hf_init()
gens = fermion.uccsd_generators(mol.nao, mol.n_elec // 2)
rng = np.random.default_rng(0)
with Statevector(ham.nbqbits) as sv:
    sv.set_hamiltonian(ham); sv.set_ucc_program(gens, hf)
    for B in (2048, 4096, 8192, 16384, 65536):
        th = rng.uniform(-.1, .1, (B, len(gens)))
        ts, en = {g: [] for g in geoms}, {}
        for r in range(reps + 1):
            for g in geoms:
                sv.set_option("sparse_shared", g)
                en[g] = sv.energy_batch(th)
                if r:
                    ts[g].append(sv.last_batch_ms())
        for g in geoms:
            t = sorted(ts[g])
            print(f"B={B:6d} sparse_shared={g}: min {t[0]:.4f} median {t[len(t) // 2]:.4f} max {t[-1]:.4f} ms -> "
                  f"{B / t[len(t) // 2] / 1e3:6.1f} M evaluations/s; max |dE| vs geometry {geoms[0]}: {np.abs(en[g] - en[geoms[0]]).max():.2e}", flush=True)
    print("geometries that ran:", sorted(sv.sparse_geometries()))
