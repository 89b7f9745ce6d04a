"""CPU tests of the deflation infrastructure (tests/deflation_cases.py): the checker against central differences of its own cost, the
declared surface, and ``excited.vqd`` on the stand-in backend."""
import os

import numpy as np
import pytest

from tests import deflation_cases as dc
from tests import gradbatch_cases as gc
from tests import hessian_cases, metric_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _central(fun, theta, h=1e-5):
    g = np.zeros(len(theta))
    for k in range(len(theta)):
        d = np.eye(len(theta))[k] * h
        g[k] = (fun(theta + d)[0] - fun(theta - d)[0]) / (2 * h)
    return g


def test_checker_against_central_differences_of_its_cost():
    """the restated adjoint pass with one ansatz vector and one random complex vector against central differences (step 1e-5) of its own
    cost, with the bound of ``test_gradbatch_cases``: 1e-8 W max(1, C) — truncation h^2 C^3 / 6 and rounding eps / h are both ~ 2e-11"""
    n, hf, rx, rz, rc, pidx, phi0, K = metric_cases.tied_program()
    tied = gc.Case(n, hf, rx, rz, rc, pidx, K, phi0=phi0, nterms=24, seed=17)
    for what, case in (("two states", gc.two_states()[0]), ("y program", gc.y_program(14, n=6)), ("tied", tied)):
        rng = np.random.default_rng(7)
        theta = rng.uniform(-0.8, 0.8, case.K)
        vectors = [dc.case_state(case, rng.uniform(-0.8, 0.8, case.K)), 0.7 * dc.random_vector(case.n, 3)]
        betas = [1.5, 2.25]
        c, g, e, o = dc.case_want(case, theta, vectors, betas)
        assert abs(c - e - sum(b * abs(x) ** 2 for b, x in zip(betas, o))) <= 1e-14 * dc.weight(case.h1, vectors, betas)
        assert abs(e - case.want(theta)[0]) <= 1e-14 * case.h1 and np.abs(o - [np.vdot(v, dc.case_state(case, theta)) for v in vectors]).max() < 1e-15
        fd = _central(lambda t: dc.case_want(case, t, vectors, betas), theta)
        worst = np.abs(fd - g).max()
        print(f"{what}: max |central differences - checker| {worst:.3e}, max |g| {np.abs(g).max():.4f}")
        assert worst <= 1e-8 * dc.weight(case.h1, vectors, betas) * max(1.0, case.C), what
        assert np.abs(g - case.want(theta)[1]).max() > 1e-3      # the penalty moves the gradient
        c0, g0, e0, o0 = dc.case_want(case, theta, [], [])         # no vectors: the undeflated checker
        assert c0 == e0 == case.want(theta)[0] and np.array_equal(g0, case.want(theta)[1]) and o0.shape == (0,)
        if what == "tied":
            assert not g[4]


def test_gate_checker_against_central_differences_of_its_cost():
    n, hf, gates, K = metric_cases.gate_list(False)
    hx, hz, hc = hessian_cases.random_real_hamiltonian(n, 16, 23)
    h1 = hessian_cases.norm1(hc, 0.1)
    C = max(sum(0.5 * abs(g[2]) for g in gates if g[4] == k) for k in range(K))
    rng = np.random.default_rng(8)
    theta = rng.uniform(-0.8, 0.8, K)
    vectors, betas = [metric_cases.gate_tangents(n, hf, gates, rng.uniform(-0.8, 0.8, K))[0], dc.random_vector(n, 4)], [2.0, 0.75]
    fun = lambda t: dc.deflated_gradient_gates(n, hf, gates, t, hx, hz, hc, 0.1, vectors, betas)   # noqa: E731
    c, g, e, o = fun(theta)
    assert np.abs(_central(fun, theta) - g).max() <= 1e-8 * dc.weight(h1, vectors, betas) * max(1.0, C)
    assert abs(e - hessian_cases.gate_hessian(n, hf, gates, theta, hx, hz, hc, 0.1)[0]) <= 1e-13 * h1


def test_symbols_are_declared_everywhere():
    from openvqe_amd import _lib, excited
    header = open(os.path.join(ROOT, "include", "ovqe_sv.h")).read()
    cdef = open(os.path.join(ROOT, "include", "ovqe_sv.cdef.h")).read()
    for name in ("ovqe_deflation_push", "ovqe_deflation_truncate", "ovqe_deflation_count", "ovqe_deflated_gradient_batch", "ovqe_deflation_info"):
        assert name + "(" in header and name + "(" in cdef and name in _lib.SIGNATURES
    assert "Out of scope: deflation on the\n * sector tables and on the partitioned register" in header and "clifford_frame" in header
    from openvqe_amd.backend import Statevector
    from openvqe_amd.evaluator import _Evaluator
    from openvqe_amd.partitioned import PartitionedStatevector
    for m in ("deflation_push", "deflation_truncate", "deflation_count", "deflated_gradient_batch", "deflation_info"):
        assert callable(getattr(Statevector, m))
        with pytest.raises(NotImplementedError):
            getattr(PartitionedStatevector, m)(None)
    assert callable(_Evaluator.deflated_gradient_batch) and callable(excited.vqd)


def check_three_levels(states, sv, found_before=0):
    """the assertions the CPU and the GPU run of the three-bit case share"""
    levels = [s["energy"] for s in states]
    print("levels", levels, "costs", [s["cost"] for s in states], "iterations", [s["result"].nit for s in states])
    assert len(states) == 3 and sv.deflation_count() == found_before
    for s, want in zip(states, dc.THREE_BIT_LEVELS):
        assert abs(s["energy"] - want) <= 1e-8, (levels, dc.THREE_BIT_LEVELS)
    for k, s in enumerate(states):
        assert s["overlaps"].shape == (found_before + k,) and s["theta"].shape == (3,) and s["result"].success
        assert np.all(np.diff(s["result"].energies) <= 0.0)
        assert abs(s["cost"] - s["energy"]) <= 1e-8 and np.abs(s["overlaps"]).max(initial=0.0) <= 1e-4    # (orthogonal to the states before it)


def test_vqd_three_levels_on_the_stand_in():
    """three index bits, H = 0.5 Z_0 + 0.8 Z_1 + 1.3 Z_2: the three lowest levels -2.6, -1.6, -1.0 within 1e-8 from the default eight
    starts; the set of vectors is what it was afterwards, also when the optimiser raises"""
    from openvqe_amd import excited
    sv = dc.DeflationOracle(3)
    dc.load_three_bits(sv)
    states = excited.vqd(sv, 3)
    check_three_levels(states, sv)
    # on top of a vector pushed before the call: the ground state as a given vector, then two levels above it
    sv.init_basis(7)    # (every Z reads -1: E = -2.6)
    sv.deflation_push(2.0 * sv.hamiltonian_norm1())
    above = excited.vqd(sv, 2)
    assert sv.deflation_count() == 1 and [s["overlaps"].shape for s in above] == [(1,), (2,)]
    assert abs(above[0]["energy"] + 1.6) <= 1e-8 and abs(above[1]["energy"] + 1.0) <= 1e-8

    def broken(X):
        raise RuntimeError("stop")

    sv.deflated_gradient_batch = broken
    with pytest.raises(RuntimeError):
        excited.vqd(sv, 1)
    assert sv.deflation_count() == 1
    with pytest.raises(ValueError):
        excited.vqd(sv, 1, x0=np.zeros(4))
