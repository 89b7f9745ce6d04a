"""the headline workload (H2O/STO-3G UCCSD, 65 536 evaluations per launch) on both geometries of the rows form in one process —
k_sparse_vqe_rows_shared (workgroup geometry, "sparse_shared" = 1) and k_sparse_vqe_rows<2> (one wave per pair of evaluations,
"sparse_shared" = 0) — each without one of its phases ("sparse_dbg": 1 no sincos, 2 no circuit rows, 3 no Hamiltonian entries; the workgroup geometry
also 4: a constant in place of every theta load): where the time goes.  5 leaves nothing out: the wave sums behind the contraction by
__shfl_down, as before sv_wave_reduce.hpp — its "phase left out" is NEGATIVE, minus the cost of the old sums.  Needs the testing build (OVQE_LIB=testing).  python tools/exp_value_phases.py [geoms=1,0] [name=value]"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from openvqe_amd import chem, fermion
from openvqe_amd.backend import Statevector
mol = chem.molecule("H2O"); mol.rhf(); ham = mol.jw_hamiltonian(); hf = mol.hf_init()
gens = fermion.uccsd_generators(mol.nao, mol.n_elec // 2)
rng = np.random.default_rng(0)
B = 65536
th = rng.uniform(-.1, .1, (B, len(gens)))
geoms = [1, 0]
with Statevector(ham.nbqbits) as sv:
    for a in sys.argv[1:]:
        k, v = a.split("=")
        if k == "geoms":
            geoms = [int(g) for g in v.split(",")]
        else:
            sv.set_option(k, int(v))
    sv.set_hamiltonian(ham); sv.set_ucc_program(gens, hf)
    whole = {}
    for geom in geoms:
        sv.set_option("sparse_shared", geom)
        for dbg, label in ((0, "whole kernel"), (1, "no sincos"), (2, "no circuit rows"), (3, "no Hamiltonian entries"),
                           (4, "no theta loads"), (5, "wave sums by __shfl_down")):
            if dbg == 4 and not geom:
                continue
            sv.set_option("sparse_dbg", dbg)
            sv.energy_batch(th)
            ts = sorted((sv.energy_batch(th), sv.last_batch_ms())[1] for _ in range(7))
            ms = ts[0]
            if dbg == 0:
                whole[geom] = ms
            print(f"sparse_shared={geom} {label:24s} {ms:7.3f} ms (median {ts[3]:.3f}, max {ts[-1]:.3f}) per {B} evaluations -> "
                  f"{B / ms * 1e3 / 1e6:6.1f} M evaluations/s; the phase left out: {whole[geom] - ms:6.3f} ms", flush=True)
    sv.set_option("sparse_dbg", 0)
    print("geometries that ran:", sorted(sv.sparse_geometries()), "forms:", sorted(sv.sparse_forms()))
    info = sv.program_info()
    print({k: info[k] for k in info if k.startswith("sp") or k in ("rotations", "support")})
