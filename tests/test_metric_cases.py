"""CPU tests of the Fubini-Study metric's checker (tests/metric_cases.py), of the natural-gradient optimiser
(openvqe_amd/common_files/natural_gradient.py) on the oracle, of the declared surface, and of the host-only plan
(openvqe_amd/csrc/sv_metric_host.hpp) replayed by tests/cpu/metric_plan_check.cpp under ASan + UBSan with g++ alone."""
import json
import os
import subprocess

import numpy as np
import pytest

from openvqe_amd import fermion
from openvqe_amd.common_files import natural_gradient
from openvqe_amd.operators import Hamiltonian, Term, pack_terms
from oracle import masks
from tests import metric_cases
from tests.oracle_backend import OracleStatevector

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _central_tangents(state, theta, h=1e-5):
    T = []
    for k in range(len(theta)):
        tp, tm = np.array(theta, float), np.array(theta, float)
        tp[k] += h
        tm[k] -= h
        T.append((state(tp) - state(tm)) / (2 * h))
    return np.array(T)


def test_checker_against_central_differences_of_oracle_states():
    """forward mode against central differences (step 1e-5) of the oracle's own states: 1e-8"""
    n, hf, rx, rz, rc, pidx, phi0, K = metric_cases.tied_program()
    theta = np.random.default_rng(3).uniform(-0.8, 0.8, K)
    psi, T = metric_cases.rotation_tangents(n, hf, rx, rz, rc, pidx, theta, phi0)
    state = lambda t: masks.ucc_state(n, hf, rx, rz, rc, pidx, t, phi0)   # noqa: E731
    assert np.abs(psi - state(theta)).max() < 1e-14
    Tn = _central_tangents(state, theta)
    assert np.abs(T - Tn).max() < 1e-8
    g = metric_cases.metric_of(psi, T)
    assert np.abs(g - metric_cases.metric_of(psi, Tn)).max() < 1e-8
    assert np.array_equal(g[4], np.zeros(K)) and np.array_equal(g[:, 4], np.zeros(K))   # the unused parameter
    assert np.linalg.eigvalsh(g)[0] > -1e-14 and np.abs(g - g.T).max() < 1e-15
    # ... and a gate list, through the stand-in backend's gate-by-gate execution
    for stray in (False, True):
        n, hf, gates, K = metric_cases.gate_list(stray)
        theta = np.random.default_rng(4).uniform(-0.8, 0.8, K)
        sv = OracleStatevector(n)
        sv.set_gate_program(gates, K, hf)

        def state(t):
            sv.prepare_state(t)
            return sv.get_state()
        psi, T = metric_cases.gate_tangents(n, hf, gates, theta)
        assert np.abs(psi - state(theta)).max() < 1e-14
        assert np.abs(T - _central_tangents(state, theta)).max() < 1e-8
        g = metric_cases.metric_of(psi, T)
        assert np.abs(g[0]).max() < 1e-15 and g[1, 1] > 0.1        # RZ on a qubit still in |0>: a zero row
    # the trailing CNOT is a fixed unitary: it drops out
    ga = metric_cases.gate_metric(*metric_cases.gate_list(False)[:3], theta)
    gb = metric_cases.gate_metric(*metric_cases.gate_list(True)[:3], theta)
    assert np.abs(ga - gb).max() < 1e-15


def test_closed_forms():
    rng = np.random.default_rng(11)
    n = 5
    # exp(-i c theta P) on psi: c^2 (1 - <P>^2); psi from constant-angle rotations in front
    strings = [("XYZ", [0, 1, 2]), ("YX", [1, 4]), ("ZY", [2, 3]), ("XZZY", [0, 2, 3, 4])]
    xz = [masks.pack_pauli(n, s, q) for s, q in strings]
    rx, rz = [x for x, _ in xz], [z for _, z in xz]
    for c in (1.0, -0.37, 2.5):
        rc, phi0 = [1.0, 1.0, 1.0, c], list(rng.uniform(-1, 1, 3)) + [0.2]
        pidx = [-1, -1, -1, 0]
        theta = [rng.uniform(-1, 1)]
        psi, T = metric_cases.rotation_tangents(n, 5, rx, rz, rc, pidx, theta, phi0)
        p = masks.expectation(psi, [rx[3]], [rz[3]], [1.0])
        g = metric_cases.metric_of(psi, T)
        assert g.shape == (1, 1) and abs(g[0, 0] - c * c * (1 - p * p)) < 1e-14
    # RY(t0) then RZ(t1) on |0>: diag(1/4, sin^2(t0)/4)
    for t0, t1 in ((0.3, -1.1), (1.2, 0.4), (0.0, 0.7)):
        g = metric_cases.gate_metric(1, 0, [("RY", [0], 1.0, 0.0, 0), ("RZ", [0], 1.0, 0.0, 1)], [t0, t1])
        assert np.abs(g - np.diag([0.25, 0.25 * np.sin(t0) ** 2])).max() < 1e-15
    # RZ on |0> alone: the <T|psi> term takes all of it
    g = metric_cases.gate_metric(1, 0, [("RZ", [0], 1.0, 0.0, 0)], [0.9])
    assert abs(g[0, 0]) < 1e-16


class MetricOracle(OracleStatevector):
    """the stand-in backend with the two calls the optimiser needs: exact gradient (adjoint method) and the checker's metric"""

    def _rot(self):
        _, xs, zs, cs, p0, pi, hf = self._prog
        return self.nbqbits, hf, xs, zs, cs, pi

    def energy_gradient(self, theta):
        hx, hz, hc, const = self._ham
        return masks.ucc_energy_gradient(*self._rot(), np.asarray(theta, float), hx, hz, hc, const, self._prog[4])

    def metric_tensor(self, theta):
        return metric_cases.rotation_metric(*self._rot(), np.asarray(theta, float), self._prog[4])


def test_natural_gradient_reaches_the_ground_energy_of_h2():
    """UCCSD on the stored H2/STO-3G Hamiltonian (K1) from theta = 0: the ground energy of that Hamiltonian within 1e-9 (UCCSD is exact
    for two electrons; the notebook's own final energy, stored next to it, lies within 1e-8 above), and the energy never rises"""
    k1 = json.load(open(os.path.join(ROOT, "tests", "golden", "k1_h2_sto3g.json")))
    H = Hamiltonian(4, [Term(c, o, q) for c, o, q in k1["terms"]], k1["constant_coeff"])
    xs, zs, cs = pack_terms(4, H.terms)
    e0 = np.linalg.eigvalsh(sum(c.real * _pauli_matrix(4, int(x), int(z)) for x, z, c in zip(xs, zs, cs)))[0] + k1["constant_coeff"]
    assert 0 <= k1["vqe_final_energy_k0000"] - e0 < 1e-8
    sv = MetricOracle(4)
    sv.set_hamiltonian(H)
    K = sv.set_ucc_program(fermion.uccsd_generators(2, 1), k1["hf_init"])
    res = natural_gradient.minimize(sv.energy_gradient, sv.metric_tensor, np.zeros(K), tol=1e-7)
    print(res.message, res.nit, res.nfev, res.fun - e0)
    assert res.success and res.nit >= 2
    assert abs(res.fun - e0) < 1e-9
    assert np.all(np.diff(res.energies) <= 0.0) and res.energies[0] == pytest.approx(-1.0716472822963232, abs=1e-13)
    assert res.x.shape == (K,) and abs(sv.energy(res.x) - res.fun) < 1e-13
    # the step itself: lambda relative to the mean diagonal, zero rows stay bounded
    g = np.diag([2.0, 0.0])
    d = natural_gradient.natural_step(g, np.array([1.0, 1.0]), damping=1e-3)
    assert np.allclose(d, [-0.5 / (2.0 + 1e-3), -0.5 / 1e-3])


def _pauli_matrix(n, x, z):
    m = np.zeros((1 << n, 1 << n), complex)
    for i in range(1 << n):
        e = np.zeros(1 << n, complex)
        e[i] = 1
        m[:, i] = masks.pauli_apply(e, x, z)
    return m


def test_metric_symbols_are_declared_everywhere():
    from openvqe_amd import _lib
    header = open(os.path.join(ROOT, "include", "ovqe_sv.h")).read()
    cdef = open(os.path.join(ROOT, "include", "ovqe_sv.cdef.h")).read()
    for name in ("ovqe_metric_tensor", "ovqe_metric_info"):
        assert name + "(" in header and name + "(" in cdef and name in _lib.SIGNATURES
    assert '"metric_workspace_mb"' in header and "O(K R) sweeps" in header
    from openvqe_amd.backend import Statevector
    from openvqe_amd.evaluator import _Evaluator
    from openvqe_amd.partitioned import PartitionedStatevector
    from openvqe_amd.ucc_family.get_energy_ucc import EnergyUCC
    for m in ("metric_tensor", "metric_info"):
        assert callable(getattr(Statevector, m))
    assert callable(_Evaluator.metric_tensor) and EnergyUCC.natural_gradient is False
    with pytest.raises(NotImplementedError):
        PartitionedStatevector.metric_tensor(None)


def test_metric_plan_under_asan_ubsan(tmp_path):
    src = os.path.join(ROOT, "tests", "cpu", "metric_plan_check.cpp")
    exe = str(tmp_path / "metric_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-o", exe, src])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    for seed in ("7", "2025"):
        r = subprocess.run([exe, seed], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "metric plan ok" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    # the programs at the limits of the compact path: the support at metric::MAX_SUPPORT, the table sizes on both sides of the staged /
    # unstaged / streaming decisions, the refusal at the first state beyond the cap
    r = subprocess.run([exe, "boundary"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "metric plan boundary ok" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    rows = [dict(f.split("=") for f in line.split()[1:]) for line in r.stdout.splitlines() if line.startswith("cube ")]
    rows = {(int(d["n"]), int(d["R"])): {k: int(v) for k, v in d.items()} for d in rows}
    table = {20: (20479, 148252, 66016, 1), 21: (22527, 156492, 66048, 2), 3669: (7493631, None, 153600, 2), 3670: (7495679, None, 153616, 0)}
    for R, (npairs, staged, unstaged, form) in table.items():
        d = rows[(12, R)]
        assert d["ok"] == 1 and (d["m"], d["ntab"], d["nops"], d["npairs"]) == (4096, R, R, npairs) == metric_cases.cube_sizes(12, R), d
        assert d["max_cj"] == 4095 and d["unstaged"] == unstaged and d["form"] == form and (staged is None or d["staged"] == staged), d
        assert d["staged"] == metric_cases.tangent_lds_bytes(d["m"], d["ntab"], d["nops"], d["npairs"], True)
        assert d["unstaged"] == metric_cases.tangent_lds_bytes(d["m"], d["ntab"], d["nops"], d["npairs"], False)
        assert metric_cases.tangent_form(d["m"], d["ntab"], d["nops"], d["npairs"])[0] == form
    assert rows[(13, 13)]["ok"] == 0 and rows[(13, 21)]["ok"] == 0


# ---- the builders of the boundary cases (tests/test_gpu_metric_edges.py) ---------------------------------------------------------------
def _support(n, hf, rx):
    """states reachable from |hf> through the x masks, in order -> sizes after each rotation"""
    S, sizes = {int(hf)}, []
    for x in rx:
        S |= {a ^ int(x) for a in S}
        sizes.append(len(S))
    return sizes


@pytest.mark.parametrize("n, R", [(6, 9), (12, 20), (12, 21), (12, 3670), (13, 21)])
def test_cube_program_fills_the_register_with_a_bounded_metric(n, R):
    """the support doubles over the first n rotations up to exactly 2^n states; every rotation is a real string with an offset (never
    fused into a pattern table); pidx covers -1..K-1; max g_kk <= 4 by the checker"""
    K = 6
    n_, hf, rx, rz, rc, pidx, phi0, K_ = metric_cases.cube_program(n, R, K, 100 + R)
    assert (n_, K_) == (n, K) and len(rx) == len(rz) == len(rc) == len(pidx) == len(phi0) == R and 0 < hf < 1 << n
    assert _support(n, hf, rx)[:n] == [2 << r for r in range(n)] and _support(n, hf, rx)[-1] == 1 << n
    ny = np.array([bin(int(x) & int(z)).count("1") for x, z in zip(rx, rz)])
    weight = np.array([bin(int(x) | int(z)).count("1") for x, z in zip(rx, rz)])
    assert np.all(ny & 1) and np.all(rx != 0) and np.all(phi0 != 0.0) and np.all(rc != 0.0)
    assert np.all(weight[:n] == 1) and np.all((weight[n:] >= 2) & (weight[n:] <= 5))
    assert set(int(p) for p in pidx) == set(range(-1, K))
    m, ntab, nops, npairs = metric_cases.cube_sizes(n, R)
    assert (m, ntab, nops) == (1 << n, R, R) and npairs == sum(s // 2 for s in _support(n, hf, rx))
    theta = np.random.default_rng(R).uniform(-0.8, 0.8, K)
    g = metric_cases.rotation_metric(n, hf, rx, rz, rc, pidx, theta, phi0)
    print(f"cube_program({n}, {R}): diag g = {np.diag(g)}")
    assert 0.01 < np.max(np.diag(g)) <= 4.0 and np.linalg.eigvalsh(g)[0] > -1e-13


def test_tangent_lds_formula_at_the_form_boundaries():
    """the byte counts of the four 12-qubit programs, from the formula of sp_metric_lds: the last staged program, the first unstaged
    one, the last that fits (its bytes EQUAL the budget) and the first that streams although a compact program exists"""
    want = {20: (20479, 148252, 66016, 1), 21: (22527, 156492, 66048, 2), 3669: (7493631, None, 153600, 2), 3670: (7495679, None, 153616, 0)}
    for R, (npairs, staged, plain, form) in want.items():
        sizes = metric_cases.cube_sizes(12, R)
        assert sizes == (4096, R, R, npairs)
        assert staged is None or metric_cases.tangent_lds_bytes(*sizes, True) == staged
        assert metric_cases.tangent_lds_bytes(*sizes, False) == plain
        assert metric_cases.tangent_form(*sizes) == (form, {1: staged, 2: plain, 0: 0}[form])
    assert metric_cases.LDS_WG_BUDGET == 153600 and metric_cases.tangent_lds_bytes(*metric_cases.cube_sizes(12, 3669), False) == 153600


@pytest.mark.parametrize("w", [7, 8])
def test_weight_program_contains_the_run_it_claims(w):
    n, hf, rx, rz, rc, pidx, phi0, K, heavy = metric_cases.weight_program(12, w)
    pop = lambda v: bin(int(v)).count("1")   # noqa: E731
    assert heavy == w + 1 and len(rx) == heavy + 4 and K == 4
    # the single-Y rotations populate every pattern of the heavy rotation: its x lies inside the bits they reached
    assert all(pop(x) == 1 and x == z for x, z in zip(rx[:heavy], rz[:heavy])) and np.all(phi0[:heavy] != 0.0)
    reached = int(np.bitwise_or.reduce(rx[:heavy]))
    assert pop(rx[heavy]) == w and int(rx[heavy]) & ~reached == 0 and int(rz[heavy]) & ~int(rx[heavy]) & reached
    assert phi0[heavy] == 0.0 and pidx[heavy] == 2 and pop(rx[heavy] & rz[heavy]) & 1
    # the run: one x, three strings, a constant between two different parameters, a new qubit in x
    run = slice(heavy + 1, heavy + 4)
    assert len(set(int(x) for x in rx[run])) == 1 and len(set(int(z) for z in rz[run])) == 3 and rx[heavy + 1] != rx[heavy]
    assert list(pidx[run]) == [3, -1, 0] and phi0[heavy + 2] != 0.0 and all(pop(x & z) & 1 for x, z in zip(rx[run], rz[run]))
    assert pop(int(rx[heavy + 1]) & ~reached) == 1
    sizes = _support(n, hf, rx)
    m, ntab, nops, npairs = metric_cases.weight_sizes(w)
    assert sizes[-1] == m == 1 << (w + 2) and sizes[heavy] == sizes[heavy - 1] == 1 << (w + 1)
    assert nops == len(rx) and ntab == nops + (63 if w == 7 else 0) and npairs == sum(s // 2 for s in sizes)
    theta = np.random.default_rng(w).uniform(-0.8, 0.8, K)
    g = metric_cases.rotation_metric(n, hf, rx, rz, rc, pidx, theta, phi0)
    assert np.all(np.diag(g) > 0.01) and np.max(np.diag(g)) <= 4.0


def test_wide_gate_list_against_central_differences_of_oracle_states():
    """the 10-qubit list of all six gates: forward mode against central differences (step 1e-5) of the stand-in backend's states: 1e-8;
    the list holds what it claims, and the stray Clifford gates drop out of g"""
    theta = np.random.default_rng(14).uniform(-0.8, 0.8, 5)
    for stray in (False, True):
        n, hf, gates, K = metric_cases.wide_gate_list(stray)
        assert n == 10 and K == 5
        sv = OracleStatevector(n)
        sv.set_gate_program(gates, K, hf)

        def state(t):
            sv.prepare_state(t)
            return sv.get_state()
        psi, T = metric_cases.gate_tangents(n, hf, gates, theta)
        assert np.abs(psi - state(theta)).max() < 1e-14
        assert np.abs(T - _central_tangents(state, theta)).max() < 1e-8
        g = metric_cases.metric_of(psi, T)
        assert np.all(np.diag(g) > 0.01) and np.linalg.eigvalsh(g)[0] > -1e-14
    n, hf, gates, K = metric_cases.wide_gate_list(False)
    have = {(name, tuple(q)) for name, q, *_ in gates}
    for name in ("H", "X", "RZ", "RY"):
        assert (name, (0,)) in have and (name, (n - 1,)) in have
    assert {"X", "H", "RX", "RY", "RZ", "CNOT"} == {name for name, *_ in gates}
    cnots = [q for name, q, *_ in gates if name == "CNOT"]
    assert any(c > t and c - t == 1 for c, t in cnots) and any(c < t and t - c == 1 for c, t in cnots)
    assert any(c > t and c - t > 4 for c, t in cnots) and any(c < t and t - c > 4 for c, t in cnots)
    assert sum(1 for _, _, s, _, p in gates if p == 1 and s == -2.0) >= 1 and sum(1 for _, _, s, _, p in gates if p == 1 and s != -2.0) >= 1
    assert any(c != 0.0 for _, _, _, c, p in gates if p >= 0) and set(p for *_, p in gates) == {-1, 0, 1, 2, 3, 4}
    ga = metric_cases.gate_metric(*metric_cases.wide_gate_list(False)[:3], theta)
    gb = metric_cases.gate_metric(*metric_cases.wide_gate_list(True)[:3], theta)
    assert np.abs(ga - gb).max() < 1e-14
