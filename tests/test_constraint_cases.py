"""CPU tests of the constraint infrastructure (tests/constraint_cases.py): the checker against central differences of its own cost, the
spin operators of ``fermion`` on dense matrices, the host-only restriction rule (openvqe_amd/csrc/sv_constrain_host.hpp) replayed by
tests/cpu/restrict_check.cpp under ASan + UBSan with g++ alone, the declared surface, and ``excited.vqd`` with a spin constraint on
the stand-in backend."""
import os
import subprocess

import numpy as np
import pytest

from oracle import masks
from tests import constraint_cases as cc
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
    """the restated adjoint pass with two observables (mixed linear and quadratic weights, a non-zero target), one ansatz vector and one
    random complex vector against central differences (step 1e-5) of its own cost, with the bound of ``test_deflation_cases``:
    1e-8 W max(1, C) — truncation h^2 C^3 / 6 and rounding eps / h are both ~ 2e-11"""
    n, hf, rx, rz, rc, pidx, phi0, K = metric_cases.tied_program()
    tied = gc.Case(n, hf, rx, rz, rc, pidx, K, phi0=phi0, nterms=24, seed=17)
    for what, case in (("two states", gc.two_states()[0]), ("y program", gc.y_program(14, n=6)), ("tied", tied)):
        rng = np.random.default_rng(7)
        theta = rng.uniform(-0.8, 0.8, case.K)
        vectors = [dc.case_state(case, rng.uniform(-0.8, 0.8, case.K)), 0.7 * dc.random_vector(case.n, 3)]
        betas = [1.5, 2.25]
        obs = [cc.pack(case.n, cc.random_observable(case.n, 10, 41, x_pool=case.rx[:64], constant=0.3)),
               cc.pack(case.n, cc.diagonal_observable(case.n, 42, constant=-0.2))]
        lin, qd, tg = [0.7, -0.4], [1.3, 0.6], [0.25, -0.5]
        c, g, e, v, o = cc.case_want(case, theta, obs, lin, qd, tg, vectors, betas)
        W = cc.weight(case.h1, obs, lin, qd, tg, vectors, betas)
        pen = sum(a * x + b * (x - t) ** 2 for a, b, t, x in zip(lin, qd, tg, v))
        c_d, g_d, e_d, o_d = dc.case_want(case, theta, vectors, betas)
        assert abs(c - c_d - pen) <= 1e-14 * W and e == e_d and np.array_equal(o, o_d)
        psi = dc.case_state(case, theta)
        for m, ob in enumerate(obs):
            assert abs(v[m] - masks.expectation(psi, ob[0], ob[1], ob[2], ob[3])) <= 1e-13 * cc.norm1(ob)
        fd = _central(lambda t: cc.case_want(case, t, obs, lin, qd, tg, vectors, betas), theta)
        worst = np.abs(fd - g).max()
        print(f"{what}: max |central differences - checker| {worst:.3e}, max |g| {np.abs(g).max():.4f}")
        assert worst <= 1e-8 * W * max(1.0, case.C), what
        assert np.abs(g - g_d).max() > 1e-3      # the observables move the gradient
        c0, g0, e0, v0, o0 = cc.case_want(case, theta, obs, None, None, None, vectors, betas)   # weights zero: the deflated checker
        assert c0 == c_d and np.array_equal(g0, g_d) and np.array_equal(v0, v)


def test_gate_checker_against_central_differences_of_its_cost():
    n, hf, gates, K = metric_cases.gate_list(False)
    hx, hz, hc = hessian_cases.random_real_hamiltonian(n, 16, 23)
    h1 = hessian_cases.norm1(hc, 0.1)
    C = max(sum(0.5 * abs(g[2]) for g in gates if g[4] == k) for k in range(K))
    rng = np.random.default_rng(8)
    theta = rng.uniform(-0.8, 0.8, K)
    vectors, betas = [dc.random_vector(n, 4)], [0.75]
    obs = [cc.pack(n, cc.random_observable(n, 8, 43, constant=0.4)), cc.pack(n, cc.diagonal_observable(n, 44))]
    lin, qd, tg = [0.5, 0.0], [-0.8, 1.1], [0.3, 0.45]
    fun = lambda t: cc.constrained_gradient_gates(n, hf, gates, t, hx, hz, hc, 0.1, obs, lin, qd, tg, vectors, betas)   # noqa: E731
    c, g, e, v, o = fun(theta)
    assert np.abs(_central(fun, theta) - g).max() <= 1e-8 * cc.weight(h1, obs, lin, qd, tg, vectors, betas) * max(1.0, C)
    assert abs(e - hessian_cases.gate_hessian(n, hf, gates, theta, hx, hz, hc, 0.1)[0]) <= 1e-13 * h1
    assert np.abs(g - dc.deflated_gradient_gates(n, hf, gates, theta, hx, hz, hc, 0.1, vectors, betas)[1]).max() > 1e-3


@pytest.mark.parametrize("n", [4, 6, 8])
def test_spin_operators_against_the_density_matrices(n):
    """``fermion.number_operator`` / ``sz_operator`` / ``spin_squared`` as dense matrices: their expectation values in a random complex
    state equal ``rdm.spin_expectations`` of the determinant oracle's density matrices of that state (``rdm_cases.vec_rdm``); S^2 commutes
    with S_z and N; its eigenvalues
    are s (s + 1)"""
    from openvqe_amd import fermion, rdm
    from oracle import dense
    from tests import rdm_cases
    ops = [fermion.number_operator(n), fermion.sz_operator(n), fermion.spin_squared(n)]
    N, Sz, S2 = [dense.operator_matrix(op, sparse=False) for op in ops]
    assert np.abs(S2 @ Sz - Sz @ S2).max() <= 1e-13 and np.abs(S2 @ N - N @ S2).max() <= 1e-13
    assert all(np.abs(np.imag([t.coeff for t in op.terms])).max() == 0.0 for op in ops)
    ev = np.linalg.eigvalsh(S2)
    s = 0.5 * (np.sqrt(1.0 + 4.0 * ev) - 1.0)
    assert np.abs(2.0 * s - np.round(2.0 * s)).max() <= 1e-10 and ev.min() > -1e-12
    psi = dc.random_vector(n, 60 + n)
    idx = np.arange(1 << n, dtype=np.uint64)       # (the determinant oracle: its own Jordan-Wigner signs, no ``fermion.jw_product``)
    g1, d2 = rdm_cases.vec_rdm(idx, psi, n, 1)[0], rdm_cases.vec_rdm(idx, psi, n, 2)[0]
    want = rdm.spin_expectations(g1, rdm.unpack_rdm2(d2, n))
    got = [float(np.real(np.vdot(psi, M @ psi))) for M in (N, Sz, S2)]
    print(n, "terms", [len(op.terms) for op in ops], "got", got, "want", want)
    assert np.abs(np.array(got) - np.array(want)).max() <= 1e-12 * n * n


# ---- the restriction rule -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def restrict_program(tmp_path_factory):
    src = os.path.join(ROOT, "tests", "cpu", "restrict_check.cpp")
    exe = str(tmp_path_factory.mktemp("restrict") / "restrict_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-o", exe, src])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")

    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
        return r.stdout

    return run


PAD = (1 << 64) - 1


def _dense_entries(n, support, xs, zs, cs):
    """the entries of the rule from the DENSE matrix of the sum: for every x in ascending order, every support state a (in the order
    given, padding skipped) with the highest bit of x clear and a ^ x in the support: Re O[a, a ^ x], doubled off the diagonal; exact
    zeros dropped.  Coefficients are multiples of 1/8: every sum is exact"""
    dim = 1 << n
    O = np.zeros((dim, dim), np.complex128)
    for b in range(dim):
        e = np.zeros(dim, np.complex128)
        e[b] = 1.0
        O[:, b] = masks.apply_pauli_sum(e, np.asarray(xs, np.uint64), np.asarray(zs, np.uint64), np.asarray(cs, np.float64))
    index = {int(a): k for k, a in enumerate(support) if int(a) != PAD}
    out = []
    for x in sorted({int(v) for v in xs}):
        for k, a in enumerate(support):
            a = int(a)
            if a == PAD or (x and a >> (x.bit_length() - 1) & 1) or (a ^ x) not in index:
                continue
            d = float(O[a, a ^ x].real)
            if d != 0.0:
                out.append((k, index[a ^ x], 2.0 * d if x else d))
    return out


def test_restriction_rule_against_a_dense_restriction(restrict_program, tmp_path):
    """random real sums on random supports (with padding slots), an operator of odd-Y terms only (no entries), an operator whose every
    partner leaves the support (diagonal entries only), the empty sum"""
    rng = np.random.default_rng(21)
    cases = []
    for trial in range(12):
        n = int(rng.integers(3, 8))
        m = int(rng.integers(1, min(40, 1 << n)))
        support = [int(a) for a in rng.choice(1 << n, size=m, replace=False)]
        for _ in range(int(rng.integers(0, 3))):
            support.insert(int(rng.integers(0, len(support) + 1)), PAD)
        T = int(rng.integers(1, 30))
        xs = [int(v) for v in rng.integers(0, 1 << n, T)]
        xs[0] = 0
        if trial % 2:       # x masks that connect support states
            xs = [0 if rng.random() < 0.3 else support[int(rng.integers(0, len(support)))] ^ support[int(rng.integers(0, len(support)))] for _ in range(T)]
            xs = [x if x < (1 << n) else 0 for x in xs]
        zs = [int(v) for v in rng.integers(0, 1 << n, T)]
        cs = [float(v) / 8.0 for v in rng.integers(-16, 17, T)]
        cases.append((n, support, xs, zs, cs))
    n = 4
    cases.append((n, [0, 1, 2, 3, 5, 9], [1, 6, 1], [1, 2, 3 | 4], [1.0, 0.5, 0.25]))          # Y_0, Y_1 X_2, Y_0 Z_1 Z_2: odd Y only
    cases.append((n, [0b0001, 0b0010, 0b0100], [0b1000, 0b1001, 0, 0b1111], [0, 0b0110, 0b0011, 0b1111 & 0b0101], [0.5, 0.25, 1.5, -0.75]))
    cases.append((n, [3, 7], [], [], []))
    lines = [str(len(cases))]
    counts = []
    for n, support, xs, zs, cs in cases:
        want = _dense_entries(n, support, xs, zs, cs)
        counts.append(len(want))
        lines.append(f"{len(support)} {len(xs)} {len(want)}")
        lines.append(" ".join(str(a) for a in support))
        lines += [f"{x} {z} {c!r}" for x, z, c in zip(xs, zs, cs)]
        lines += [f"{i} {j} {c!r}" for i, j, c in want]
    path = tmp_path / "restrict_cases.txt"
    path.write_text("\n".join(lines) + "\n")
    out = restrict_program(path)
    print(out)
    assert out.count(" ok") == len(cases)
    assert counts[-3] == 0 and counts[-1] == 0                       # odd Y only; the empty sum
    assert counts[-2] == 3 and max(counts[:12]) > 10                 # every partner outside: the diagonal alone


def test_symbols_are_declared_everywhere():
    from openvqe_amd import _lib, excited, fermion
    header = open(os.path.join(ROOT, "include", "ovqe_sv.h")).read()
    cdef = open(os.path.join(ROOT, "include", "ovqe_sv.cdef.h")).read()
    names = ("ovqe_observable_push", "ovqe_observable_truncate", "ovqe_observable_count", "ovqe_constrained_gradient_batch", "ovqe_constraint_info")
    for name in names:
        assert name + "(" in header and name + "(" in cdef and name in _lib.SIGNATURES
    assert "Out of scope: constraints on the sector tables and on the\n * partitioned register, open Clifford frames, a constrained Hessian or metric, per-row weights" in header
    lib = os.path.join(ROOT, "openvqe_amd", "lib", "libovqe_sv.so")
    if os.path.exists(lib):
        exported = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
        for name in names:
            assert f" T {name}\n" in exported, name
    from openvqe_amd.backend import Statevector
    from openvqe_amd.partitioned import PartitionedStatevector
    for m in ("observable_push", "observable_truncate", "observable_count", "constrained_gradient_batch", "expectations_batch", "constraint_info"):
        assert callable(getattr(Statevector, m))
        with pytest.raises(NotImplementedError):
            getattr(PartitionedStatevector, m)(None)
    assert callable(excited.spin_constraint) and callable(fermion.spin_squared)
    op, target, weight = excited.spin_constraint(4, 1.0)
    assert target == 2.0 and weight is None and op.nbqbits == 4
    for src in ("sv_constrain_host.hpp", "constrain_host.inc", "abi_constrain.inc"):
        assert os.path.exists(os.path.join(ROOT, "openvqe_amd", "csrc", src))
    assert "constrain::restrict_to_support(h->ham.groups" in open(os.path.join(ROOT, "openvqe_amd", "csrc", "sparse_host.inc")).read()


# ---- spin-pure VQD ------------------------------------------------------------------------------------------------------------------------
# what the stand-in reached (the reference of tests/test_gpu_constraints.py::test_flow_spin_pure_vqd)
H2_TRIPLET = -0.76266          # the lowest S = 1 level of chem.molecule("H2") in the sector of |hf>, by dense diagonalisation
STAND_IN_S2 = 7.58e-3          # <S^2> of state 1 of the constrained run


def test_vqd_with_a_spin_constraint_on_the_stand_in():
    """``chem.molecule("H2")`` (8 qubits, UCCSD, K = 15), three starts.  Dense levels in the sector of |hf>: -1.15169 (S^2 = 0), -0.76266
    (2), -0.59218 (0).  Measured on the stand-in:
        unconstrained   state 0  E -1.1516885475  <S^2> 1.3e-14      state 1  E -0.6708891443  <S^2> 1.010   (426 iterations)
        constrained     state 0  E -1.1516885475  <S^2> 6.7e-16      state 1  E -0.3373413922  <S^2> 7.578e-3 (157 iterations)
    (eight starts, the default: the same two minima, -0.6708891444 / 1.010 and -0.3373414037 / 7.579e-3).  The spin-orbital UCCSD
    generators do not conserve S^2: unconstrained, state 1 is an open-shell mixture of singlet and triplet, <S^2> just above 1, below
    every excited singlet; the constraint removes the triplet part.  The handle's observables and vectors are what they were afterwards,
    also when the optimiser raises"""
    from openvqe_amd import excited, fermion
    from tests import spread_cases
    case = spread_cases.molecule("H2")
    n = case.n
    sv = cc.ConstraintOracle(n)
    sv.set_hamiltonian(case.ham)
    sv.set_ucc_program(case.gens, case.hf)
    sv.observable_push(fermion.number_operator(n))       # held before the call: enters with weight zero, is still there afterwards
    plain = excited.vqd(sv, 2, starts=3)
    assert sv.observable_count() == 1 and sv.deflation_count() == 0 and "values" not in plain[0]
    sv.observable_push(fermion.spin_squared(n))
    _, values = sv.expectations_batch(np.array([s["theta"] for s in plain]))
    sv.observable_truncate(1)
    print("unconstrained", [(s["energy"], v[1]) for s, v in zip(plain, values)], [s["result"].nit for s in plain])
    assert abs(values[0, 1]) <= 1e-8 and values[1, 1] > 1.0
    assert np.abs(values[:, 0] - 2.0).max() <= 1e-10
    pure = excited.vqd(sv, 2, starts=3, constraints=[excited.spin_constraint(n, 0.0)])
    print("constrained", [(s["energy"], s["cost"], s["values"]) for s in pure], [s["result"].nit for s in pure])
    assert sv.observable_count() == 1 and sv.deflation_count() == 0
    for k, s in enumerate(pure):
        assert s["result"].success and np.all(np.diff(s["result"].energies) <= 0.0)
        assert s["values"].shape == (2,) and abs(s["values"][0] - 2.0) <= 1e-10 and s["overlaps"].shape == (k,)
        assert abs(s["values"][1]) <= 10.0 * STAND_IN_S2
    assert abs(pure[0]["energy"] - plain[0]["energy"]) <= 1e-8
    assert pure[1]["energy"] >= H2_TRIPLET - 1e-9 and pure[1]["energy"] > plain[1]["energy"]

    def broken(X, **kwargs):
        raise RuntimeError("stop")

    sv.constrained_gradient_batch = broken
    with pytest.raises(RuntimeError):
        excited.vqd(sv, 1, constraints=[excited.spin_constraint(n, 0.0)])
    assert sv.observable_count() == 1 and sv.deflation_count() == 0
