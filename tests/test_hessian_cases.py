"""CPU tests of the energy Hessian's checkers (tests/hessian_cases.py), of the Newton trust-region optimiser
(openvqe_amd/common_files/newton.py) on the oracle, of the declared surface, and of the host-only plan
(openvqe_amd/csrc/sv_hessian_host.hpp) replayed by tests/cpu/hessian_plan_check.cpp under ASan + UBSan with g++ alone."""
import json
import os
import subprocess

import numpy as np
import pytest

from openvqe_amd import fermion
from openvqe_amd.backend import compile_ucc_program
from openvqe_amd.common_files import newton
from openvqe_amd.operators import Hamiltonian, Term, pack_terms
from oracle import masks
from tests import hessian_cases, metric_cases
from tests.oracle_backend import OracleStatevector

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _k1():
    k1 = json.load(open(os.path.join(ROOT, "tests", "golden", "k1_h2_sto3g.json")))
    H = Hamiltonian(4, [Term(c, o, q) for c, o, q in k1["terms"]], k1["constant_coeff"])
    xs, zs, cs = pack_terms(4, H.terms)
    return k1, H, xs, zs, np.real(cs)


def _central_hessian(grad, theta, h=1e-5):
    K = len(theta)
    out = np.zeros((K, K))
    for k in range(K):
        tp, tm = np.array(theta, float), np.array(theta, float)
        tp[k] += h
        tm[k] -= h
        out[k] = (grad(tp) - grad(tm)) / (2 * h)
    return out


def _cases():
    n, hf, rx, rz, rc, pidx, phi0, K = metric_cases.tied_program()
    hx, hz, hc = hessian_cases.random_real_hamiltonian(n, 24, 17)
    yield "tied program", (n, hf, rx, rz, rc, pidx), np.random.default_rng(3).uniform(-0.8, 0.8, K), (hx, hz, hc, 0.3), phi0
    k1, _, xs, zs, cs = _k1()
    rx, rz, rc, rp, K = compile_ucc_program(4, fermion.uccsd_generators(2, 1))
    yield "H2 UCCSD", (4, k1["hf_init"], rx, rz, rc, rp), np.array([0.05, -0.03, -0.1137]), (xs, zs, cs, k1["constant_coeff"]), None


def test_checker_against_central_differences_of_the_oracle_gradient():
    """nested forward mode against central differences (step 1e-5) of ``masks.ucc_energy_gradient``: 1e-7 ||H||_1.  The truncation term
    h^2 times the fourth derivative over 6 and the rounding term eps / h = 2e-11 both lie below 1e-9 ||H||_1 here, which is asserted
    as well (1.3e-11 and 1.0e-10 ||H||_1 are measured): the bound keeps two orders of margin.  The adjoint form agrees with the nested
    one to rounding, and E and the gradient with the oracle's."""
    for what, prog, theta, (hx, hz, hc, const), phi0 in _cases():
        h1 = hessian_cases.norm1(hc)
        e, g, hs = hessian_cases.rotation_hessian(*prog, theta, hx, hz, hc, const, phi0)
        e0, g0 = masks.ucc_energy_gradient(*prog, theta, hx, hz, hc, const, phi0)
        assert abs(e - e0) < 1e-13 * h1 and np.abs(g - g0).max() < 1e-13 * h1
        cd = _central_hessian(lambda t: masks.ucc_energy_gradient(*prog, t, hx, hz, hc, const, phi0)[1], theta)
        err = np.abs(hs - cd).max()
        print(f"{what}: max|H - central| = {err:.3e} = {err / h1:.2e} ||H||_1, max|H| = {np.abs(hs).max():.4f}")
        assert err <= 1e-7 * h1 and np.abs(hs).max() > 0.05 * h1 / 10
        assert err <= 1e-9 * h1   # truncation and rounding confirmed: two orders inside the bound
        assert np.array_equal(hs, hs.T)
        ea, ga, ha, asym = hessian_cases.rotation_hessian_adjoint(*prog, theta, hx, hz, hc, const, phi0)
        print(f"   adjoint form: max|delta| = {np.abs(ha - hs).max():.3e}, asymmetry {asym:.3e}")
        assert abs(ea - e) < 1e-13 * h1 and np.abs(ga - g).max() < 1e-13 * h1
        assert np.abs(ha - hs).max() < 1e-12 * h1 and asym < 1e-12 * h1
    # the tied program's unused parameter: an exact zero row and column
    what, prog, theta, (hx, hz, hc, const), phi0 = next(_cases())
    hs = hessian_cases.rotation_hessian(*prog, theta, hx, hz, hc, const, phi0)[2]
    assert not hs[4].any() and not hs[:, 4].any() and abs(hs[0, 0]) > 1e-3


def test_adjoint_form_against_the_nested_form_at_mid_size():
    """the O(K) adjoint form, the reference of the cases whose second tangents do not fit a test (LiH, K = 65 on 12 qubits), held to
    the nested forward mode where both run at a size of that kind: H4/STO-3G UCCSD (8 qubits, K = 26, 160 rotations, tied parameters) with
    its own Hamiltonian, and 65 rotations with a parameter each on 8 qubits with a random real Hamiltonian on the program's masks:
    1e-12 ||H||_1 max(1, C^2) — rounding of 1e3 to 1e4 additions per entry at 2e-16 each, two orders of margin"""
    from openvqe_amd import chem
    mol = chem.molecule("H4")
    mol.rhf()
    ham = mol.jw_hamiltonian()
    n = ham.nbqbits
    hfv = mol.hf_init()
    hf = int(hfv) if np.isscalar(hfv) else int(sum(1 << (n - 1 - q) for q, v in enumerate(hfv) if v))
    rx, rz, rc, rp, K = compile_ucc_program(n, fermion.uccsd_generators(mol.nao, mol.n_elec // 2))
    hx, hz, hc = pack_terms(n, ham.terms)
    cases = [("H4 UCCSD", (n, hf, rx, rz, rc, rp), K, (hx, hz, np.real(hc), float(np.real(ham.constant_coeff or 0.0))), 0.3)]
    _, gens, hf2 = fermion.synthetic_molecule(4, 2, 41)
    rx, rz, rc, rp = metric_cases.one_parameter_per_rotation(gens, 8, 65)
    hx, hz, hc = hessian_cases.random_real_hamiltonian(8, 20, 365, x_pool=rx)
    cases.append(("65 parameters on 8 qubits", (8, hf2, rx, rz, rc, rp), 65, (hx, hz, hc, 0.25), 0.4))
    for what, prog, K, (hx, hz, hc, const), spread in cases:
        assert (K * K) << prog[0] <= hessian_cases.NESTED_LIMIT
        theta = np.random.default_rng(K).uniform(-spread, spread, K)
        h1 = hessian_cases.norm1(hc, const)
        C = hessian_cases.coefficient_sum(prog[4], prog[5], K)
        e, g, hs = hessian_cases.rotation_hessian(*prog, theta, hx, hz, hc, const)
        ea, ga, ha, asym = hessian_cases.rotation_hessian_adjoint(*prog, theta, hx, hz, hc, const)
        tol = 1e-12 * h1 * max(1.0, C * C)
        print(f"{what}: K = {K}, max|adjoint - nested| = {np.abs(ha - hs).max():.3e}, asymmetry {asym:.3e}, tol {tol:.3e}, "
              f"max|H| = {np.abs(hs).max():.3f}")
        assert abs(ea - e) <= 1e-13 * h1 and np.abs(ga - g).max() <= tol
        assert np.abs(ha - hs).max() <= tol and asym <= tol and np.abs(hs).max() > 0.01


def test_gate_checker_against_central_differences():
    """the gate-list checker against central differences of the stand-in backend's energies' gradient (second differences of E at
    step 1e-4: 1e-6 ||H||_1), closed frame and open frame"""
    hx, hz, hc = hessian_cases.random_real_hamiltonian(5, 16, 23)
    h1 = hessian_cases.norm1(hc)
    for stray in (False, True):
        n, hf, gates, K = metric_cases.gate_list(stray)
        theta = np.random.default_rng(4).uniform(-0.8, 0.8, K)
        e, g, hs = hessian_cases.gate_hessian(n, hf, gates, theta, hx, hz, hc, 0.1)

        def energy(t):
            psi, _ = metric_cases.gate_tangents(n, hf, gates, t)
            return masks.expectation(psi, hx, hz, hc, 0.1)
        assert abs(e - energy(theta)) < 1e-13 * h1
        h = 1e-4
        for b in range(K):
            for k in range(b, K):
                eb, ek = np.eye(K)[b] * h, np.eye(K)[k] * h
                cd = (energy(theta + eb + ek) - energy(theta + eb - ek) - energy(theta - eb + ek) + energy(theta - eb - ek)) / (4 * h * h)
                assert abs(hs[b, k] - cd) <= 1e-6 * h1, (b, k, hs[b, k], cd)
        assert np.abs(hs[0]).max() < 1e-14 * h1 and abs(hs[1, 1]) > 1e-3   # RZ on a qubit still in |0>: a zero row


def test_closed_form_of_one_rotation():
    """exp(-i c theta P) behind constant rotations: E'' = -4 c^2 (E - (<H>_0 + <P H P>_0) / 2), the index 0 for the state in front of
    the rotation: 1e-13 ||H||_1"""
    rng = np.random.default_rng(11)
    n = 5
    strings = [("XYZ", [0, 1, 2]), ("YX", [1, 4]), ("ZY", [2, 3]), ("XZZY", [0, 2, 3, 4])]
    xz = [masks.pack_pauli(n, s, q) for s, q in strings]
    rx, rz = [x for x, _ in xz], [z for _, z in xz]
    hx, hz, hc = hessian_cases.random_real_hamiltonian(n, 20, 5)
    h1 = hessian_cases.norm1(hc)
    for c in (1.0, -0.37, 2.5):
        rc, phi0 = [1.0, 1.0, 1.0, c], list(rng.uniform(-1, 1, 3)) + [0.2]
        pidx = [-1, -1, -1, 0]
        theta = [rng.uniform(-1, 1)]
        e, g, hs = hessian_cases.rotation_hessian(n, 5, rx, rz, rc, pidx, theta, hx, hz, hc, 0.0, phi0)
        psi0 = masks.ucc_state(n, 5, rx[:3], rz[:3], rc[:3], pidx[:3], theta, phi0[:3])
        ppsi = masks.pauli_apply(psi0, rx[3], rz[3])
        mid = 0.5 * (masks.expectation(psi0, hx, hz, hc) + masks.expectation(ppsi, hx, hz, hc))
        assert hs.shape == (1, 1) and abs(hs[0, 0] + 4 * c * c * (e - mid)) <= 1e-13 * h1


class HessianOracle(OracleStatevector):
    """the stand-in backend with the one call the optimiser needs, from the checker"""

    def energy_hessian(self, theta):
        _, xs, zs, cs, p0, pi, hf = self._prog
        hx, hz, hc, const = self._ham
        return hessian_cases.rotation_hessian(self.nbqbits, hf, xs, zs, cs, pi, np.asarray(theta, float), hx, hz, hc, const, p0)


def test_newton_reaches_the_ground_energy_of_h2():
    """UCCSD on the stored H2/STO-3G Hamiltonian (K1) from theta = 0 by trust-region Newton steps: the ground energy of that Hamiltonian
    within 1e-9, one device call per distinct point, the accepted energies never rise, the solution is a minimum"""
    k1, H, xs, zs, cs = _k1()
    e0 = np.linalg.eigvalsh(sum(c * _pauli_matrix(4, int(x), int(z)) for x, z, c in zip(xs, zs, cs)))[0] + k1["constant_coeff"]
    sv = HessianOracle(4)
    sv.set_hamiltonian(H)
    K = sv.set_ucc_program(fermion.uccsd_generators(2, 1), k1["hf_init"])
    calls = []

    def fgh(theta):
        calls.append(np.array(theta))
        return sv.energy_hessian(theta)
    res = newton.minimize(fgh, np.zeros(K), tol=1e-8)
    print(res.message, res.nit, res.ncalls, res.fun - e0, res.lowest_eigenvalue)
    assert res.success and res.nit >= 2 and abs(res.fun - e0) < 1e-9
    assert np.linalg.norm(res.jac) <= 1e-8 and res.lowest_eigenvalue >= -1e-8
    assert np.all(np.diff(res.energies) <= 0.0) and res.energies[0] == pytest.approx(-1.0716472822963232, abs=1e-13)
    assert res.ncalls == len(calls) and len({c.tobytes() for c in calls}) == len(calls)   # no point evaluated twice
    assert abs(sv.energy(res.x) - res.fun) < 1e-13
    none = newton.minimize(lambda t: (1.5, np.zeros(0), np.zeros((0, 0))), np.zeros(0))   # no parameter: the energy alone
    assert none.success and none.fun == 1.5 and none.energies == [1.5]


def _pauli_matrix(n, x, z):
    m = np.zeros((1 << n, 1 << n), complex)
    for i in range(1 << n):
        e = np.zeros(1 << n, complex)
        e[i] = 1
        m[:, i] = masks.pauli_apply(e, x, z)
    return m


def test_stability_of_a_saddle():
    low, vec = newton.stability(np.diag([2.0, -1.0]))
    assert low == -1.0 and np.allclose(np.abs(vec), [0.0, 1.0])
    assert newton.stability(np.array([[2.0, 0.0], [0.0, 0.5]]))[0] == 0.5
    assert newton.stability(np.zeros((0, 0)))[0] == 0.0


def test_hessian_symbols_are_declared_everywhere():
    from openvqe_amd import _lib
    header = open(os.path.join(ROOT, "include", "ovqe_sv.h")).read()
    cdef = open(os.path.join(ROOT, "include", "ovqe_sv.cdef.h")).read()
    for name in ("ovqe_energy_hessian", "ovqe_hessian_info"):
        assert name + "(" in header and name + "(" in cdef and name in _lib.SIGNATURES
    assert "reproduces to rounding, not to the bit" in header and "O(K R) sweeps" in header.split("ovqe_metric_info(")[1]
    from openvqe_amd.backend import Statevector
    from openvqe_amd.evaluator import _Evaluator
    from openvqe_amd.partitioned import PartitionedStatevector
    from openvqe_amd.ucc_family.get_energy_ucc import EnergyUCC
    for m in ("energy_hessian", "hessian_info"):
        assert callable(getattr(Statevector, m))
    assert callable(_Evaluator.energy_hessian) and EnergyUCC.newton is False
    with pytest.raises(NotImplementedError):
        PartitionedStatevector.energy_hessian(None)


def test_lds_formula_restated():
    """the boundaries of the cube programs at m = 4096: four vectors of 4096 doubles leave 22 KiB of the 150 KiB budget"""
    assert hessian_cases.hessian_lds_bytes(441, 1000, 140, 0, 0, False) == (4 * 442 * 8 + 40000 + 1120 + 15) // 16 * 16
    a, b, c, d = hessian_cases.cube_boundaries(12, 6)
    assert (a, b, c, d) == (12, 13, 562, 563)
    form = lambda R: hessian_cases.hessian_form(*hessian_cases._cube(12, R, 6))   # noqa: E731
    assert [form(R)[0] for R in (a, b, c, d)] == [1, 2, 2, 0] and form(c)[1] <= 150 * 1024 < form(c)[1] + 40


def test_hessian_plan_under_asan_ubsan(tmp_path):
    src = os.path.join(ROOT, "tests", "cpu", "hessian_plan_check.cpp")
    exe = str(tmp_path / "hessian_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-o", exe, src])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    for seed in ("7", "2025"):
        r = subprocess.run([exe, seed], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "hessian plan ok" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    r = subprocess.run([exe, "boundary"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "hessian plan boundary ok" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    rows = [dict(f.split("=") for f in line.split()[1:]) for line in r.stdout.splitlines() if line.startswith("cube ")]
    bounds = hessian_cases.cube_boundaries(12, 6)
    assert [int(row["R"]) for row in rows if row["n"] == "12"] == list(bounds)
    for row in rows:
        if row["n"] != "12":
            assert row["ok"] == "0"   # the first support beyond the cap
            continue
        sizes = (int(row["m"]), int(row["ntab"]), 6, int(row["nops"]), int(row["npairs"]))
        assert sizes == hessian_cases._cube(12, int(row["R"]), 6)
        assert int(row["staged"]) == hessian_cases.hessian_lds_bytes(*sizes, True)
        assert int(row["unstaged"]) == hessian_cases.hessian_lds_bytes(*sizes, False)
        assert int(row["form"]) == hessian_cases.hessian_form(*sizes)[0]
    assert [int(row["form"]) for row in rows if row["n"] == "12"] == [1, 2, 2, 0]
