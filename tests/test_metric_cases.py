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
