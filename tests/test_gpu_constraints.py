"""GPU tests of the observables beside the Hamiltonian (ovqe_observable_push / _truncate / _count, ovqe_constrained_gradient_batch,
ovqe_constraint_info: k_sparse_constrained_batch in csrc/sv_sparse.hpp, csrc/sv_constrain_host.hpp, constrain_host.inc,
abi_constrain.inc) and of spin-pure variational quantum deflation on top of them (openvqe_amd/excited.py: vqd(constraints=...)).

Bounds (tests/constraint_cases.py): with W = ||H||_1 + sum_j beta_j ||phi_j||^2 + sum_m (|linear_m| + 2 |quad_m| (||O_m||_1 + |target_m|))
||O_m||_1 and C of tests/gradbatch_cases.py, 1e-10 W max(1, C) against the checker, 1e-12 W max(1, C) against another call on the same
handle; a value o_bm 1e-10 ||O_m||_1 against the checker and 1e-12 ||O_m||_1 against another call.  Every path-1 call is also held to
``gradbatch_cases.check_info`` through the info entries it shares with ovqe_gradient_batch_info."""
import ctypes

import numpy as np
import pytest

from openvqe_amd import excited, fermion
from tests import constraint_cases as cc
from tests import deflation_cases as dc
from tests import gradbatch_cases as gc
from tests import hessian_cases, metric_cases
from tests.test_gpu_deflation import Held, _molecule, _same_bits, _sizes

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
INVALID, STATE = -1, -5


@pytest.fixture(scope="module")
def SV(gpu_lib):
    from openvqe_amd.backend import Statevector
    return Statevector


@pytest.fixture(scope="module")
def h4():
    return _molecule("H4")


@pytest.fixture(scope="module")
def lih():
    return _molecule("LiH")


class Obs:
    """the observables a handle holds, as the checker sees them, with the weights of the calls"""

    def __init__(self):
        self.ops, self.packed = [], []
        self.linear = self.quad = self.target = None

    def push(self, sv, n, op):
        assert sv.observable_push(op) == len(self.ops) + 1
        self.ops.append(op)
        self.packed.append(cc.pack(n, op))

    def weights(self, linear=None, quad=None, target=None):
        self.linear, self.quad, self.target = linear, quad, target
        return self

    def args(self):
        return self.packed, self.linear, self.quad, self.target


def _call(sv, thetas, obs, held):
    """constrained_gradient_batch with the checks every result gets -> (costs, grads, energies, values, overlaps, info)"""
    thetas = np.ascontiguousarray(thetas, np.float64)
    c, g, e, v, o = sv.constrained_gradient_batch(thetas, obs.linear, obs.quad, obs.target)
    info = sv.constraint_info()
    B, K = thetas.shape
    M, J = len(obs.ops), len(held.vectors)
    assert c.shape == e.shape == (B,) and g.shape == (B, K) and v.shape == (B, M) and o.shape == (B, J)
    assert all(np.all(np.isfinite(a)) for a in (c, g, e, v, o.view(np.float64)))
    assert (info["B"], info["K"], info["M"], info["J"]) == (B, K, M, J) and sv.observable_count() == M and sv.deflation_count() == J, info
    lin, qd, tg = cc._weights(M, obs.linear, obs.quad, obs.target)
    pen = np.array([sum(b * abs(x) ** 2 for b, x in zip(held.betas, row)) for row in o]).reshape(B)
    pen = pen + (v * lin).sum(axis=1) + (qd * (v - tg) ** 2).sum(axis=1)
    assert np.abs(c - e - pen).max() <= 1e-13 * cc.weight(1.0, *obs.args(), held.vectors, held.betas)   # the cost is that of the returned values
    return c, g, e, v, o, info


def _against_checker(case, obs, held, thetas, out, rows, want=None):
    c, g, e, v, o = out[:5]
    tol = cc.bound_checker(case.h1, case.C, *obs.args(), held.vectors, held.betas)
    for b in rows:
        cw, gw, ew, vw, ow = cc.case_want(case, thetas[b], *obs.args(), held.vectors, held.betas) if want is None else want(thetas[b])
        dcost, de, dg = abs(c[b] - cw), abs(e[b] - ew), float(np.abs(g[b] - gw).max(initial=0.0))
        dv = [abs(x - y) for x, y in zip(v[b], vw)]
        print(f"   row {b} against the checker: |dC| {dcost:.3e} |dE| {de:.3e} max|dg| {dg:.3e} bound {tol:.3e}; values {[f'{x:.1e}' for x in dv]}; "
              f"penalty {cw - ew:.4f} max|g| {np.abs(gw).max(initial=0.0):.4f}")
        assert dcost <= tol and de <= tol and dg <= tol
        for x, ob in zip(dv, obs.packed):
            assert x <= cc.bound_value(ob)
        for x, y, vec in zip(o[b], ow, held.vectors):
            assert abs(x - y) <= dc.bound_overlap(vec)


def _path1(sv, info, K, B, waves=0, workgroups=0, sizes=None):
    sizes = _sizes(sv, info, K) if sizes is None else sizes
    gc.check_info(info, sizes, B, waves=waves, workgroups=workgroups)
    return sizes


def _spin_ops(n):
    return [fermion.spin_squared(n), fermion.number_operator(n), fermion.sz_operator(n)]


# ---- path 1 ------------------------------------------------------------------------------------------------------------------------------
def test_no_observables_is_the_deflated_call(SV, h4):
    """H4, B = 9, M = 0 with the weights NULL, one vector held: costs, energies and overlaps are ovqe_deflated_gradient_batch's to the
    bit, gradients within the same-handle bound"""
    thetas = np.random.default_rng(70).uniform(-0.3, 0.3, (9, h4.K))
    held, obs = Held(), Obs()
    with SV(h4.n) as sv:
        sv.set_hamiltonian(h4.ham)
        sv.set_ucc_program(h4.gens, h4.hf)
        held.push_ansatz(sv, thetas[4], 1.5)
        c0, g0, e0, o0 = sv.deflated_gradient_batch(thetas)
        out = _call(sv, thetas, obs, held)
        _path1(sv, out[5], h4.K, 9)
    c, g, e, v, o, info = out
    print(info)
    assert info["entries"] == 0 and info["rows"] == 1 and v.shape == (9, 0)
    assert _same_bits(c, c0) and _same_bits(e, e0) and _same_bits(o.view(np.float64), o0.view(np.float64))
    assert np.abs(g - g0).max() <= dc.bound_single(h4.h1, h4.C, held.vectors, held.betas)


def test_hamiltonian_as_its_own_observable(SV, h4):
    """H pushed as observable 0 with linear = 1: the values are the energies, the cost 2 E, the gradient twice the plain one"""
    thetas = np.random.default_rng(71).uniform(-0.3, 0.3, (5, h4.K))
    held, obs = Held(), Obs().weights(linear=[1.0])
    with SV(h4.n) as sv:
        sv.set_hamiltonian(h4.ham)
        sv.set_ucc_program(h4.gens, h4.hf)
        obs.push(sv, h4.n, h4.ham)
        e0, g0 = sv.energy_gradient_batch(thetas)
        out = _call(sv, thetas, obs, held)
        _path1(sv, out[5], h4.K, 5)
        assert out[5]["entries"] > 0
    c, g, e, v, o, info = out
    tol = cc.bound_single(h4.h1, h4.C, *obs.args())
    print(info, "max |v - e|", np.abs(v[:, 0] - e).max(), "max |c - 2e|", np.abs(c - 2 * e).max(), "max |g - 2 g0|", np.abs(g - 2 * g0).max(), "bound", tol)
    assert np.abs(e - e0).max() <= tol and np.abs(v[:, 0] - e).max() <= cc.bound_value(obs.packed[0], other_call=True)
    assert np.abs(c - 2.0 * e).max() <= tol and np.abs(g - 2.0 * g0).max() <= tol


@pytest.mark.parametrize("which", ["no_active_op", "two_states"])
def test_smallest_supports(SV, which):
    """m = 1 and m = 2 with an observable of odd-Y terms only: no restricted entry, the value is its constant on every row, and the
    gradient under a quadratic weight is the weight-zero call's to the bit"""
    case, _ = getattr(gc, which)()
    thetas = np.random.default_rng(len(which)).uniform(-0.6, 0.6, (3, case.K))
    held, obs = Held(), Obs()
    with SV(case.n) as sv:
        case.load(sv)
        obs.push(sv, case.n, cc.odd_y_only(case.n, constant=0.5))
        zero = _call(sv, thetas, obs, held)
        out = _call(sv, thetas, obs.weights(linear=[0.25], quad=[1.3], target=[0.2]), held)
        _path1(sv, out[5], case.K, 3)
    print(f"{which}: {out[5]}")
    assert out[5]["support"] == (1 if which == "no_active_op" else 2) and out[5]["entries"] == 0
    assert np.all(out[3] == 0.5) and np.all(zero[3] == 0.5)
    assert _same_bits(out[1], zero[1]) and _same_bits(out[2], zero[2])
    assert np.abs(out[0] - out[2] - (0.25 * 0.5 + 1.3 * 0.09)).max() <= 1e-14
    _against_checker(case, obs, held, thetas, out, range(3))


def test_more_than_one_trip_per_lane(SV):
    """``fermion.synthetic_molecule(5, 2, 7)`` at 10 qubits: up to 100 support states in 128 slots — two trips per lane, padding slots the
    restriction skips (between 33 and 4064 states the slots are a multiple of 32, so the slot count itself is always even).  S^2, N and
    S_z with non-zero targets and mixed weights, two deflation vectors, one complex: every row against the checker"""
    from openvqe_amd.backend import compile_ucc_program
    ham, gens, hf = fermion.synthetic_molecule(5, 2, 7)
    n = 10
    rx, rz, rc, rp, K = compile_ucc_program(n, gens)
    case = gc.Case(n, hf, rx, rz, rc, rp, K, ham=ham)
    thetas = np.random.default_rng(72).uniform(-0.3, 0.3, (4, K))
    held, obs = Held(), Obs().weights(linear=[0.3, -0.2, 0.0], quad=[1.5, 0.0, 0.7], target=[0.75, 0.0, 0.5])
    with SV(n) as sv:
        sv.set_hamiltonian(ham)
        sv.set_ucc_program(gens, hf)
        for op in _spin_ops(n):
            obs.push(sv, n, op)
        held.push_ansatz(sv, thetas[3], 1.25)
        held.push_vector(sv, dc.random_vector(n, 73), 0.75)
        out = _call(sv, thetas, obs, held)
        sizes = _path1(sv, out[5], K, 4)
    info = out[5]
    print(info)
    assert 64 < info["support"] <= 100 and sizes[0] == 128 and gc.slots(info["support"]) != info["support"] and info["rows"] == 3
    assert info["entries"] > 128 and info["restriction_builds"] == 3
    assert np.abs(out[3][:, 1] - 4.0).max() <= 1e-12 and np.abs(out[3][:, 2]).max() <= 1e-12     # UCCSD keeps N and S_z
    assert np.abs(out[3][:, 0]).max() > 1e-4                                                      # ... but not S^2
    _against_checker(case, obs, held, thetas, out, range(4))


@pytest.fixture(scope="module")
def lih_rows(lih):
    return np.random.default_rng(12).uniform(-0.2, 0.2, (41, lih.K))


@pytest.mark.parametrize("nw", [1, 2, 4, 8])
def test_lih_every_wave_count(SV, lih, lih_rows, nw):
    """LiH UCCSD (m = 225 in 256 slots, K = 92) under "grad_batch_waves" = nw with M = 2 (S^2 with a quadratic, N with a linear weight)
    and one complex vector: B = nw + 1 — the second workgroup has waves without a row — and B = 5 nw + 1 on two workgroups — second and
    third trips.  Equal rows at different positions give equal bits"""
    held, obs = Held(), Obs().weights(linear=[0.0, 0.4], quad=[2.0, 0.0], target=[0.1, 0.0])
    with SV(lih.n) as sv:
        sv.set_option("grad_batch_waves", nw)
        sv.set_hamiltonian(lih.ham)
        sv.set_ucc_program(lih.gens, lih.hf)
        obs.push(sv, lih.n, fermion.spin_squared(lih.n))
        obs.push(sv, lih.n, fermion.number_operator(lih.n))
        held.push_vector(sv, dc.random_vector(lih.n, 77), 2.5)
        sizes = None
        for B, wgs in ((nw + 1, 0), (5 * nw + 1, 2)):
            sv.set_option("grad_batch_workgroups", wgs)
            thetas = lih_rows[:B].copy()
            thetas[B - 1] = thetas[0]
            out = _call(sv, thetas, obs, held)
            c, g, e, v, o, info = out
            sizes = _path1(sv, info, lih.K, B, waves=nw, workgroups=wgs, sizes=sizes)
            print(f"LiH nw = {nw} B = {B}: {info}")
            assert info["support"] == 225 and info["waves"] == nw and info["rows"] == 2
            assert info["workgroups"] == (2 if wgs else -(-B // nw)) and info["restriction_builds"] == (0 if wgs else 2)
            assert _same_bits(c[0], c[B - 1]) and _same_bits(e[0], e[B - 1]) and _same_bits(v[0], v[B - 1])
            assert _same_bits(o[0].view(np.float64), o[B - 1].view(np.float64))
            _against_checker(lih, obs, held, thetas, out, [1] if wgs == 0 else [B - 2])
            tol = cc.bound_single(lih.h1, lih.C, *obs.args(), held.vectors, held.betas)
            for b in (0, B - 1):
                c1, g1, e1, v1, o1 = sv.constrained_gradient_batch(thetas[b:b + 1], obs.linear, obs.quad, obs.target)
                assert abs(c1[0] - c[b]) <= tol and np.abs(g1[0] - g[b]).max() <= tol
                assert all(abs(x - y) <= cc.bound_value(ob, other_call=True) for x, y, ob in zip(v1[0], v[b], obs.packed))


@pytest.mark.parametrize("which", ["two_staged", "two_plain"])
def test_both_kernel_forms(SV, which):
    """m = 4096 on 12 qubits (every lane owns 64 slots) on both sides of the staging boundary, M = 1"""
    R = gc.y_boundaries()[which]
    case, sizes = gc.y_program(R), gc.y_sizes(R)
    thetas = np.random.default_rng(R).uniform(-0.7, 0.7, (3, case.K))
    held, obs = Held(), Obs().weights(linear=[-0.3], quad=[0.8], target=[0.4])
    with SV(case.n) as sv:
        case.load(sv)
        obs.push(sv, case.n, cc.random_observable(case.n, 12, 75, x_pool=case.rx[:64], constant=0.2))
        out = _call(sv, thetas, obs, held)
        _path1(sv, out[5], case.K, 3, sizes=sizes)
    print(f"{which} R = {R}: {out[5]}")
    assert out[5]["form"] == (1 if which == "two_staged" else 2) and out[5]["entries"] > 1000
    _against_checker(case, obs, held, thetas, out, [1])


def test_zero_weight_branch(SV, h4):
    """M = 8, the cap, with weights on observable 5 alone: the gradients are those of the call that holds that observable alone, and
    ``values`` is filled for all eight"""
    thetas = np.random.default_rng(76).uniform(-0.3, 0.3, (3, h4.K))
    ops = [cc.random_observable(h4.n, 10, 80 + m, x_pool=h4.rx[:64], constant=0.1 * m) for m in range(8)]
    ops[5] = fermion.spin_squared(h4.n)
    held = Held()
    with SV(h4.n) as sv:
        sv.set_hamiltonian(h4.ham)
        sv.set_ucc_program(h4.gens, h4.hf)
        one = Obs().weights(linear=[0.5], quad=[1.5], target=[0.3])
        one.push(sv, h4.n, ops[5])
        first = _call(sv, thetas, one, held)
        sv.observable_truncate(0)
        lin, qd, tg = np.zeros(8), np.zeros(8), np.zeros(8)
        lin[5], qd[5], tg[5] = 0.5, 1.5, 0.3
        full = Obs().weights(linear=lin, quad=qd, target=tg)
        for op in ops:
            full.push(sv, h4.n, op)
        out = _call(sv, thetas, full, held)
        _path1(sv, out[5], h4.K, 3)
    assert out[5]["M"] == 8 and out[5]["restriction_builds"] == 8
    tol = cc.bound_single(h4.h1, h4.C, *one.args())
    assert np.abs(out[1] - first[1]).max() <= tol and np.abs(out[0] - first[0]).max() <= tol
    assert np.abs(out[3][:, 5] - first[3][:, 0]).max() <= cc.bound_value(one.packed[0], other_call=True)
    _against_checker(h4, full, held, thetas, out, [0, 2])


def test_entry_cache(SV, h4):
    """the observables are restricted when their set or the compact program changed, and only then"""
    thetas = np.random.default_rng(3).uniform(-0.3, 0.3, (2, h4.K))
    held, obs = Held(), Obs().weights(quad=[1.0, 0.5])
    with SV(h4.n) as sv:
        sv.set_hamiltonian(h4.ham)
        sv.set_ucc_program(h4.gens, h4.hf)
        obs.push(sv, h4.n, fermion.spin_squared(h4.n))
        obs.push(sv, h4.n, fermion.sz_operator(h4.n))
        assert _call(sv, thetas, obs, held)[5]["restriction_builds"] == 2
        assert _call(sv, thetas, obs, held)[5]["restriction_builds"] == 0
        sv.observable_truncate(1)
        del obs.ops[1:], obs.packed[1:]
        obs.weights(quad=[1.0, 0.5])
        obs.push(sv, h4.n, fermion.number_operator(h4.n))
        out = _call(sv, thetas, obs, held)
        assert out[5]["restriction_builds"] == 2
        _against_checker(h4, obs, held, thetas, out, [0])
        assert _call(sv, thetas, obs, held)[5]["restriction_builds"] == 0
        sv.set_ucc_program(h4.gens, h4.hf)
        out = _call(sv, thetas, obs, held)
        assert out[5]["restriction_builds"] == 2 and out[5]["path"] == 1
        _against_checker(h4, obs, held, thetas, out, [1])


# ---- path 2 ------------------------------------------------------------------------------------------------------------------------------
def _path2(info):
    assert info["path"] == 2 and info["launches"] > 0, info
    assert not any(info[k] for k in ("rows", "form", "waves", "workgroups", "lds_bytes", "support", "entries", "restriction_builds")), info


def test_path_2_forced_on_h4_and_path_1_agrees(SV, h4):
    """"force_path" 2 on H4 with M = 2 and three vectors against the checker; the same rows on path 1 agree within the checker's bound"""
    thetas = np.random.default_rng(9).uniform(-0.3, 0.3, (3, h4.K))
    outs = []
    for path in (2, 0):
        held, obs = Held(), Obs().weights(linear=[0.2, -0.6], quad=[1.1, 0.0], target=[0.5, 0.0])
        with SV(h4.n) as sv:
            sv.set_option("force_path", path)
            sv.set_hamiltonian(h4.ham)
            sv.set_ucc_program(h4.gens, h4.hf)
            obs.push(sv, h4.n, fermion.spin_squared(h4.n))
            obs.push(sv, h4.n, cc.random_observable(h4.n, 12, 90, x_pool=h4.rx[:64], constant=-0.3))
            held.push_ansatz(sv, thetas[1], 2.0)
            for j in range(2):
                held.push_vector(sv, dc.random_vector(h4.n, 20 + j, real=j == 1), 0.5 + j)
            out = _call(sv, thetas, obs, held)
            if path == 2:
                _path2(out[5])
                again = _call(sv, thetas, obs, held)
                assert all(_same_bits(a.view(np.float64), b.view(np.float64)) for a, b in zip(out[:5], again[:5]))
            else:
                _path1(sv, out[5], h4.K, 3)
        _against_checker(h4, obs, held, thetas, out, range(3))
        outs.append((out, obs, held))
    (a, obs, held), (b, _, _) = outs
    tol = cc.bound_checker(h4.h1, h4.C, *obs.args(), held.vectors, held.betas)
    assert np.abs(a[0] - b[0]).max() <= tol and np.abs(a[1] - b[1]).max() <= tol and np.abs(a[2] - b[2]).max() <= tol
    assert all(np.abs(a[3][:, m] - b[3][:, m]).max() <= cc.bound_value(ob) for m, ob in enumerate(obs.packed))


def test_path_2_tied_program(SV):
    """a complex program with a constant rotation, an offset, a tied and an unused parameter: the unused column is exact zeros"""
    n, hf, rx, rz, rc, pidx, phi0, K = metric_cases.tied_program()
    case = gc.Case(n, hf, rx, rz, rc, pidx, K, phi0=phi0, nterms=24, seed=17)
    thetas = np.random.default_rng(5).uniform(-0.8, 0.8, (3, K))
    held, obs = Held(), Obs().weights(linear=[0.7, -0.4], quad=[1.3, 0.6], target=[0.25, -0.5])
    with SV(n) as sv:
        case.load(sv)
        obs.push(sv, n, cc.random_observable(n, 10, 41, x_pool=rx[:64], constant=0.3))
        obs.push(sv, n, cc.odd_y_only(n, constant=-0.2))          # (a complex state: the odd-Y terms count on the full register)
        held.push_vector(sv, dc.random_vector(n, 6), 2.0)
        out = _call(sv, thetas, obs, held)
        _path2(out[5])
    _against_checker(case, obs, held, thetas, out, range(3))
    assert not out[1][:, 4].any()


def test_path_2_literal_gate_list(SV):
    n, hf, gates, K = metric_cases.gate_list(False)
    hx, hz, hc = hessian_cases.random_real_hamiltonian(n, 16, 23)
    ham = hessian_cases.hamiltonian_object(n, hx, hz, hc, 0.1)

    class G:
        h1 = hessian_cases.norm1(hc, 0.1)
        C = max(sum(0.5 * abs(g[2]) for g in gates if g[4] == k) for k in range(K))

    thetas = np.random.default_rng(6).uniform(-0.8, 0.8, (3, K))
    held, obs = Held(), Obs().weights(linear=[0.5, 0.0], quad=[-0.8, 1.1], target=[0.3, 0.45])
    with SV(n) as sv:
        sv.set_option("clifford_frame", 0)
        sv.set_hamiltonian(ham)
        sv.set_gate_program(gates, K, hf)
        assert sv.program_info()["literal_gates"] > 0
        obs.push(sv, n, cc.random_observable(n, 8, 43, constant=0.4))
        obs.push(sv, n, cc.diagonal_observable(n, 44))
        held.push_vector(sv, dc.random_vector(n, 9), 0.5)
        out = _call(sv, thetas, obs, held)
        _path2(out[5])
    _against_checker(G, obs, held, thetas, out, range(3),
                     want=lambda t: cc.constrained_gradient_gates(n, hf, gates, t, hx, hz, hc, 0.1, *obs.args(), held.vectors, held.betas))


def test_path_2_seventeen_qubits(SV):
    """the 17-qubit program of tests/stream_cases.py (one qubit past the compact path), M = 2, one row against the checker"""
    from tests import stream_cases as st
    case = st.boundary_pair()[1]
    thetas = np.ascontiguousarray(st.thetas(case, 1, 31), np.float64).reshape(1, case.K)
    held, obs = Held(), Obs().weights(linear=[0.4, 0.0], quad=[0.0, 0.9], target=[0.0, 0.35])
    with SV(case.n) as sv:
        case.load(sv)
        obs.push(sv, case.n, cc.random_observable(case.n, 10, 91, x_pool=case.rx[:64], constant=0.2))
        obs.push(sv, case.n, cc.diagonal_observable(case.n, 92))
        out = _call(sv, thetas, obs, held)
        _path2(out[5])
    _against_checker(case, obs, held, thetas, out, [0])


# ---- contract ----------------------------------------------------------------------------------------------------------------------------
def _raw(sv, B, theta, K, M, linear, quad, target, costs, grads, energies, values, overlaps):
    rc = sv._L.ovqe_constrained_gradient_batch(sv._h, B, theta, K, M, linear, quad, target, costs, grads, energies, values, overlaps)
    return rc, (sv._L.ovqe_last_error(sv._h) or b"").decode()


@pytest.mark.parametrize("path", [1, 2])
def test_bounds_of_the_arrays(SV, h4, path):
    """theta with a NaN tail, the five outputs with sentinel tails: finite results, untouched sentinels"""
    B, K, J, M = 5, h4.K, 2, 2
    rows = np.random.default_rng(15).uniform(-0.3, 0.3, (B, K))
    theta = np.concatenate([rows.reshape(-1), np.full(3 * K, np.nan)])
    costs, energies, grads = np.full(B + 16, SENTINEL), np.full(B + 16, SENTINEL), np.full(B * K + 64, SENTINEL)
    values, overlaps = np.full(B * M + 16, SENTINEL), np.full(2 * B * J + 32, SENTINEL)
    lin, qd, tg = np.array([0.3, 0.0, np.nan]), np.array([0.0, 1.2, np.nan]), np.array([0.0, 0.5, np.nan])
    held, obs = Held(), Obs().weights(lin[:2], qd[:2], tg[:2])
    with SV(h4.n) as sv:
        sv.set_option("force_path", 2 if path == 2 else 0)
        sv.set_hamiltonian(h4.ham)
        sv.set_ucc_program(h4.gens, h4.hf)
        obs.push(sv, h4.n, fermion.spin_squared(h4.n))
        obs.push(sv, h4.n, fermion.number_operator(h4.n))
        held.push_ansatz(sv, rows[0], 1.0)
        held.push_vector(sv, dc.random_vector(h4.n, 2), 2.0)
        rc, msg = _raw(sv, B, theta, K, M, lin, qd, tg, costs, grads, energies, values, overlaps)
        assert rc == 0, msg
        assert sv.constraint_info()["path"] == path
        c, g, e, v, o, _ = _call(sv, rows, obs, held)
    for arr, used in ((costs, B), (energies, B), (grads, B * K), (values, B * M), (overlaps, 2 * B * J)):
        assert np.all(np.isfinite(arr[:used])) and np.all(arr[used:] == SENTINEL)
    tol = cc.bound_single(h4.h1, h4.C, *obs.args(), held.vectors, held.betas)
    assert np.abs(costs[:B] - c).max() <= tol and np.abs(grads[:B * K] - g.reshape(-1)).max() <= tol
    assert np.abs(values[:B * M] - v.reshape(-1)).max() <= 1e-12 * max(cc.norm1(ob) for ob in obs.packed)


def test_refusals_and_the_empty_batch(SV):
    n, hf, rx, rz, rc, pidx, phi0, K = metric_cases.tied_program()
    case = gc.Case(n, hf, rx, rz, rc, pidx, K, phi0=phi0, nterms=24, seed=17)
    theta, c, e, g = np.zeros(2 * K), np.full(2, SENTINEL), np.full(2, SENTINEL), np.full(2 * K, SENTINEL)
    v, o = np.full(16, SENTINEL), np.full(8, SENTINEL)
    w = np.zeros(8)

    def refused(sv, code, text, *args):
        rc, msg = _raw(sv, *args)
        assert rc == code and text in msg, (rc, msg)

    def last(sv):
        return (sv._L.ovqe_last_error(sv._h) or b"").decode()

    op = cc.diagonal_observable(n, 1, constant=0.5)
    xs, zs, cs, const = cc.pack(n, op)
    with SV(n) as sv:
        info = (ctypes.c_int64 * 16)(*([7] * 16))
        assert sv._L.ovqe_constraint_info(sv._h, info, 16) == 0 and not any(info)          # zeros before the first call
        refused(sv, STATE, "no program set", 2, theta, K, 0, None, None, None, c, g, e, v, o)
        sv.set_rotation_program(rx, rz, rc, pidx, K, hf, phi0=phi0)
        refused(sv, STATE, "no Hamiltonian set", 2, theta, K, 0, None, None, None, c, g, e, v, o)
        sv.set_hamiltonian(case.ham)
        refused(sv, INVALID, "K does not match", 2, theta, K - 1, 0, None, None, None, c, g, e, v, o)
        refused(sv, INVALID, "B is negative", -1, theta, K, 0, None, None, None, c, g, e, v, o)
        refused(sv, INVALID, "theta is NULL", 2, None, K, 0, None, None, None, c, g, e, v, o)
        refused(sv, INVALID, "costs is NULL", 2, theta, K, 0, None, None, None, None, g, e, v, o)
        refused(sv, INVALID, "grads is NULL", 2, theta, K, 0, None, None, None, c, None, e, v, o)
        refused(sv, INVALID, "the handle holds 0 observables", 2, theta, K, 1, w, w, w, c, g, e, v, o)
        sv.set_option("real_state", 1)
        refused(sv, STATE, "real_state", 2, theta, K, 0, None, None, None, c, g, e, v, o)
        assert sv._L.ovqe_observable_push(sv._h, len(xs), xs, zs, cs, const) == STATE and "real_state" in last(sv)
        sv.set_option("real_state", 0)
        # the observables: the ninth, not finite, beyond the register, truncation at its edges
        count = ctypes.c_int32(-1)
        assert sv._L.ovqe_observable_count(sv._h, ctypes.byref(count)) == 0 and count.value == 0
        assert sv._L.ovqe_observable_truncate(sv._h, 0) == 0 and sv._L.ovqe_observable_truncate(sv._h, 1) == INVALID and "outside 0 .. 0" in last(sv)
        assert sv._L.ovqe_observable_push(sv._h, len(xs), xs, zs, cs, np.nan) == INVALID and "constant" in last(sv)
        assert sv._L.ovqe_observable_push(sv._h, 1, np.array([1 << n], np.uint64), np.zeros(1, np.uint64), np.ones(1), 0.0) == INVALID
        for m in range(8):
            assert sv.observable_push(op) == m + 1
        assert sv._L.ovqe_observable_push(sv._h, len(xs), xs, zs, cs, const) == INVALID and "at most 8" in last(sv) and sv.observable_count() == 8
        assert sv._L.ovqe_observable_truncate(sv._h, 9) == INVALID and "outside 0 .. 8" in last(sv)
        refused(sv, INVALID, "the handle holds 8 observables", 2, theta, K, 7, w, w, w, c, g, e, v, o)
        sv.observable_truncate(2)
        assert sv.observable_count() == 2
        for k, name in enumerate(("linear", "quad", "target")):
            for bad in (np.nan, np.inf):
                args = [w.copy(), w.copy(), w.copy()]
                args[k][1] = bad
                refused(sv, INVALID, "observable 1 is not finite", 2, theta, K, 2, *args, c, g, e, v, o)
        assert sv._L.ovqe_constraint_info(sv._h, info, 16) == 0 and not any(info)          # refused calls leave no figures
        # B = 0: OVQE_OK, nothing touched, NULL arrays allowed
        assert _raw(sv, 0, None, K, 2, None, None, None, None, None, None, None, None)[0] == 0
        assert _raw(sv, 0, theta, K, 2, w, w, w, c, g, e, v, o)[0] == 0
        assert all(np.all(a == SENTINEL) for a in (c, g, e, v, o))
        assert sv._L.ovqe_constraint_info(sv._h, info, 16) == 0 and not any(info)
        out = sv.constrained_gradient_batch(np.zeros((0, K)))
        assert [a.shape for a in out] == [(0,), (0, K), (0,), (0, 2), (0, 0)]
        # energies, values and overlaps may be NULL; weights NULL: the expectation values of a batch
        assert _raw(sv, 2, theta, K, 2, None, None, None, c, g, None, None, None)[0] == 0 and np.all(c != SENTINEL) and np.all(e == SENTINEL) and np.all(v == SENTINEL)
        assert sv._L.ovqe_constraint_info(sv._h, info, 16) == 0 and list(info)[:6] == [2, 2, K, 2, 0, 0]
        assert sv._L.ovqe_constraint_info(sv._h, info, -1) == INVALID and sv._L.ovqe_constraint_info(sv._h, None, 16) == INVALID
        e2, v2 = sv.expectations_batch(np.zeros((2, K)))
        assert v2.shape == (2, 2) and np.all(np.isfinite(v2)) and _same_bits(e2, np.array(c))
        with pytest.raises(ValueError):
            sv.constrained_gradient_batch(np.zeros((2, K)), quad=[1.0])
        for bad in (np.zeros(K), np.zeros((2, K + 1))):
            with pytest.raises(ValueError):
                sv.constrained_gradient_batch(bad)
    with SV(n - 1, n_global=1, shard_index=0) as shard:
        assert shard._L.ovqe_observable_push(shard._h, len(xs), xs, zs, cs, const) == STATE and "shard" in last(shard)
        rc, msg = _raw(shard, 2, theta, K, 0, None, None, None, c, g, e, v, o)
        assert rc != 0 and rc == shard._L.ovqe_energy_gradient_batch(shard._h, 2, theta, K, e, g), (rc, msg)


def test_open_clifford_frame_is_refused(SV):
    n, hf, gates, K = metric_cases.gate_list(True)
    hx, hz, hc = hessian_cases.random_real_hamiltonian(n, 16, 23)
    theta, c, g, v = np.zeros(K), np.zeros(1), np.zeros(K), np.zeros(1)
    w = np.zeros(1)
    with SV(n) as sv:
        sv.set_hamiltonian(hessian_cases.hamiltonian_object(n, hx, hz, hc, 0.1))
        sv.set_gate_program(gates, K, hf)
        sv.observable_push(cc.diagonal_observable(n, 44))
        rc, msg = _raw(sv, 1, theta, K, 1, w, w, w, c, g, None, v, None)
        assert rc == STATE and "clifford_frame" in msg and "open" in msg, (rc, msg)
        sv.set_option("clifford_frame", 0)
        sv.set_gate_program(gates, K, hf)
        rc, msg = _raw(sv, 1, theta, K, 1, w, w, w, c, g, None, v, None)
        assert rc == 0, msg
    want = cc.constrained_gradient_gates(n, hf, gates, theta, hx, hz, hc, 0.1, [cc.pack(n, cc.diagonal_observable(n, 44))])
    assert abs(c[0] - want[0]) <= 1e-10 * hessian_cases.norm1(hc, 0.1) and abs(v[0] - want[3][0]) <= 1e-10 * n


@pytest.mark.parametrize("path", [0, 2])
def test_neighbours_untouched(SV, h4, path):
    """cached tables stay valid: energy, energy_gradient, energy_gradient_batch, deflated_gradient_batch and spread_gradient_batch
    before and after a constrained call return the same bits (the gradients, added by atomics on path 1, within 1e-13 ||H||_1);
    the observables survive a new Hamiltonian and program"""
    theta = np.random.default_rng(9).uniform(-0.3, 0.3, h4.K)
    thetas = np.random.default_rng(10).uniform(-0.3, 0.3, (7, h4.K))
    held, obs = Held(), Obs().weights(linear=[0.3, 0.0], quad=[0.0, 1.5], target=[0.0, 0.75])

    def neighbours(sv):
        eb, gb = sv.energy_gradient_batch(thetas)
        cd, gd, ed, od = sv.deflated_gradient_batch(thetas)
        cs, gs, es, ss = sv.spread_gradient_batch(thetas, w_energy=0.5)
        e1, g1 = sv.energy_gradient(theta)
        return [np.array([sv.energy(theta), e1]), eb, cd, ed, od.view(np.float64), cs, es, ss], [g1, gb, gd, gs]

    with SV(h4.n) as sv:
        sv.set_option("force_path", path)
        sv.set_hamiltonian(h4.ham)
        sv.set_ucc_program(h4.gens, h4.hf)
        held.push_ansatz(sv, theta, 2.0)
        before = neighbours(sv)
        forms = sv.sparse_forms()
        obs.push(sv, h4.n, fermion.number_operator(h4.n))
        obs.push(sv, h4.n, fermion.spin_squared(h4.n))
        first = _call(sv, thetas, obs, held)
        assert first[5]["path"] == (2 if path == 2 else 1)
        after = neighbours(sv)
        if path == 0:
            assert sv.sparse_forms() == forms
        sv.set_hamiltonian(h4.ham)
        sv.set_ucc_program(h4.gens, h4.hf)
        assert sv.observable_count() == 2 and sv.deflation_count() == 1
        out = _call(sv, thetas, obs, held)
    for a, b in zip(before[0], after[0]):
        assert _same_bits(a, b)
    scales = [h4.h1, h4.h1, dc.weight(h4.h1, held.vectors, held.betas), h4.h1 * max(1.0, h4.h1)]     # (the spread's operator is quadratic in H)
    for a, b, scale in zip(before[1], after[1], scales):
        assert np.abs(a - b).max() <= 1e-13 * scale * max(1.0, h4.C)
    assert _same_bits(first[0], out[0]) and _same_bits(first[3], out[3])
    _against_checker(h4, obs, held, thetas, out, [1])


# ---- spin-pure VQD -----------------------------------------------------------------------------------------------------------------------
def test_flow_spin_pure_vqd(SV):
    """``chem.molecule("H2")`` (8 qubits, UCCSD, K = 15), the molecule of tests/test_constraint_cases.py, whose docstring holds the
    stand-in's figures: unconstrained, state 1 of ``vqd(sv, 2)`` is the open-shell mixture with <S^2> = 1.010 (> 1); with
    ``spin_constraint(n, 0.0)`` the stand-in reached <S^2> = 7.58e-3 on state 1, so the threshold here is ten times that, 7.58e-2 (the
    factor allows for another L-BFGS trajectory under rounding; the floor of 1e-8 does not bind).  State 1 lies at or above the dense
    triplet level -0.76266 (every singlet above the ground state does).  Accepted costs never rise, every returned theta is stationary
    to the tolerance in a single-row call, the returned values are a fresh evaluation's, the handle holds what it held"""
    from tests.test_constraint_cases import H2_TRIPLET, STAND_IN_S2
    case = _molecule("H2")
    n, tol = case.n, 1e-6
    threshold = max(10.0 * STAND_IN_S2, 1e-8)
    s2 = fermion.spin_squared(n)
    with SV(n) as sv:
        sv.set_hamiltonian(case.ham)
        sv.set_ucc_program(case.gens, case.hf)
        sv.observable_push(s2)                               # held before the calls: read through expectations_batch, weight zero in vqd
        plain = excited.vqd(sv, 2)
        assert sv.observable_count() == 1 and sv.deflation_count() == 0
        _, values = sv.expectations_batch(np.array([s["theta"] for s in plain]))
        print(f"unconstrained: energies {[s['energy'] for s in plain]} <S^2> {values[:, 0]} iterations {[s['result'].nit for s in plain]}")
        assert abs(values[0, 0]) <= 1e-8 and values[1, 0] > 1.0
        weight = 2.0 * sv.hamiltonian_norm1()
        pure = excited.vqd(sv, 2, constraints=[excited.spin_constraint(n, 0.0)], tol=tol)
        assert sv.constraint_info()["path"] == 1 and sv.observable_count() == 1 and sv.deflation_count() == 0
        print(f"constrained: energies {[s['energy'] for s in pure]} costs {[s['cost'] for s in pure]} <S^2> {[s['values'][1] for s in pure]} "
              f"threshold {threshold:.3e} iterations {[s['result'].nit for s in pure]}; {sv.constraint_info()}")
        sv.observable_push(s2)                               # what vqd held while it ran
        held, obs = Held(), Obs().weights(quad=[0.0, weight], target=[0.0, 0.0])
        obs.ops, obs.packed = [s2, s2], [cc.pack(n, s2)] * 2
        for k, s in enumerate(pure):
            assert s["result"].success and np.all(np.diff(s["result"].energies) <= 0.0)
            assert s["overlaps"].shape == (k,) and s["values"].shape == (2,)
            c, g, e, v, o, _ = _call(sv, s["theta"][None, :], obs, held)
            assert np.abs(g).max() <= tol
            bound = cc.bound_single(case.h1, case.C, *obs.args(), held.vectors, held.betas)
            assert abs(c[0] - s["cost"]) <= bound and abs(e[0] - s["energy"]) <= bound
            assert np.abs(v[0] - s["values"]).max() <= cc.bound_value(obs.packed[0], other_call=True)
            assert abs(s["values"][1]) <= threshold
            held.push_ansatz(sv, s["theta"], weight)
        assert pure[1]["energy"] >= H2_TRIPLET - 1e-9
        sv.deflation_truncate(0)
        sv.observable_truncate(1)
        assert sv.observable_count() == 1 and sv.deflation_count() == 0
