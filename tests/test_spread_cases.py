"""CPU tests of the energy spread's infrastructure (tests/spread_cases.py): the checker against central differences of its own cost, the
restated LDS layout, planner and closure rule against the host-only header (openvqe_amd/csrc/sv_spread_host.hpp) replayed by
tests/cpu/spread_plan_check.cpp under ASan + UBSan with g++ alone, the declared surface, and ``excited.folded_spectrum`` on the
stand-in backend."""
import os
import subprocess

import numpy as np
import pytest

from oracle import masks
from tests import gradbatch_cases as gc
from tests import spread_cases as sp
from tests.util import support_closure

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def h2():
    return sp.molecule("H2")


def _central(fun, theta, h=1e-5):
    g = np.zeros(len(theta))
    for k in range(len(theta)):
        d = np.eye(len(theta))[k] * h
        g[k] = (fun(theta + d)[0] - fun(theta - d)[0]) / (2 * h)
    return g


def test_checker_against_central_differences_on_h2(h2):
    """H2 / 6-31G (8 qubits, K = 15), both modes, mixed weights: the checker's gradient against central differences (step 1e-5) of its own
    cost at 1e-7.  In variance mode the differences move omega = E with theta: the gradient at fixed omega is the exact one all the same"""
    assert (h2.n, h2.K) == (8, 15)
    rng = np.random.default_rng(3)
    theta = rng.uniform(-0.4, 0.4, h2.K)
    e0 = sp.case_want(h2, theta)[2]
    for omega, we, ws in ((None, 0.0, 1.0), (None, 0.3, 1.0), (e0 + 0.4, 0.0, 1.0), (e0 - 0.2, 0.3, 1.0), (None, 1.0, 0.0)):
        cost, g, e, s = sp.case_want(h2, theta, omega, we, ws)
        fd = _central(lambda t: sp.case_want(h2, t, omega, we, ws), theta)
        worst = np.abs(fd - g).max()
        print(f"omega {omega} weights ({we}, {ws}): E {e:.8f} S {s:.3e} max |central differences - checker| {worst:.3e} max |g| {np.abs(g).max():.4f}")
        assert worst <= 1e-7
        assert abs(cost - we * e - ws * s) <= 1e-14 * max(1.0, abs(cost)) and abs(e - h2.want(theta)[0]) <= 1e-13 * h2.h1 and s >= 0.0
        if ws == 0.0:
            assert np.abs(g - h2.want(theta)[1]).max() <= 1e-13 * h2.h1
    # the variance against the dense matrix: <H^2> - <H>^2
    from oracle import dense
    H = dense.operator_matrix(h2.ham)
    psi = masks.ucc_state(h2.n, h2.hf, h2.rx, h2.rz, h2.rc, h2.pidx, theta)
    var = float(np.vdot(psi, H @ (H @ psi)).real - np.vdot(psi, H @ psi).real ** 2)
    assert abs(sp.case_want(h2, theta)[3] - var) <= 1e-12 * h2.h1 ** 2


def test_checker_on_a_gate_list_against_central_differences():
    from tests import hessian_cases, metric_cases
    n, hf, gates, K = metric_cases.gate_list(False)
    hx, hz, hc = hessian_cases.random_real_hamiltonian(n, 16, 23)
    theta = np.random.default_rng(8).uniform(-0.8, 0.8, K)
    for omega in (None, 0.35):
        fun = lambda t: sp.spread_gradient_gates(n, hf, gates, t, hx, hz, hc, 0.1, omega, 0.3, 1.0)   # noqa: E731
        assert np.abs(_central(fun, theta) - fun(theta)[1]).max() <= 1e-7 * sp.operator_norm(hc, 0.1, omega, 0.3, 1.0)


# ---- layout and planner ------------------------------------------------------------------------------------------------------------------
def test_restated_layout():
    """the three-array region: LiH-like and m = 4096 (96 KiB of state arrays), and where the two kernels part"""
    assert sp.wave_stride(256, 1100, 92) == gc.wave_stride(256, 1100, 92) + 256 * 8
    assert sp.wave_stride(4096, 14, 24) == 3 * 32768 + 14 * 24 + 24 * 8
    one = sp.plan(*gc.y_sizes(14), 3)
    assert (one["nw"], one["stage"], one["per_cu"]) == (1, True, 1)        # one wave per workgroup, one workgroup per CU; the 32 KiB of pair words fit beside it
    last, first = sp.y_lds_boundary()
    assert sp.plan(*gc.y_sizes(last), 3) is not None and sp.plan(*gc.y_sizes(first), 3) is None and gc.plan(*gc.y_sizes(first), 3) is not None
    assert sp.wave_stride(*[gc.y_sizes(last)[k] for k in (0, 1, 4)]) <= 150 * 1024 < sp.wave_stride(*[gc.y_sizes(first)[k] for k in (0, 1, 4)])


def _planner_cases():
    last, first = sp.y_lds_boundary()
    cases = [gc.y_sizes(R) + (3, 0, 0, 256) for R in (14, last, first)]
    lih, h2o = (256, 1100, 700, 6000, 92), (448, 2500, 1500, 20000, 140)
    # (1024 slots: LDS, not registers, bounds the residency — the staged form wins its ties at two and four waves)
    for sizes in (lih, h2o, (70, 160, 100, 700, 26), (1, 2, 0, 0, 1), (2, 1, 1, 1, 1), (128, 9, 9, 400, 9), (1024, 30, 30, 200, 10)):
        for B in (1, 3, 64, 4096):
            cases.append(sizes + (B, 0, 0, 256))
        for nw in gc.WAVES:
            for B in (1, nw - 1, nw, nw + 1, 5 * nw + 1):
                if B >= 1:
                    cases.append(sizes + (B, nw, 0, 256))
            cases.append(sizes + (5 * nw + 1, nw, 2, 256))
        cases.append(sizes + (100000, 0, 0, 8))
        cases.append(sizes + (7, 3, 0, 256))
    rng = np.random.default_rng(12)
    for _ in range(200):
        cases.append((int(rng.integers(1, 4097)), int(rng.integers(1, 5000)), int(rng.integers(0, 3000)), int(rng.integers(0, 40000)),
                      int(rng.integers(1, 300)), int(rng.integers(1, 5000)), int(rng.choice([0, 0, 1, 2, 4, 8])), int(rng.choice([0, 0, 1, 7, 300])),
                      int(rng.choice([1, 8, 256, 304]))))
    return cases


@pytest.fixture(scope="module")
def check_program(tmp_path_factory):
    src = os.path.join(ROOT, "tests", "cpu", "spread_plan_check.cpp")
    exe = str(tmp_path_factory.mktemp("spread") / "spread_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-o", exe, src])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")

    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
        return r.stdout

    return run


def test_planner_under_asan_ubsan(check_program, tmp_path):
    cases = _planner_cases()
    listing = tmp_path / "cases.txt"
    listing.write_text("".join(" ".join(str(v) for v in c) + "\n" for c in cases))
    out = check_program(listing)
    assert f"spread plan ok ({len(cases)} cases)" in out
    rows = [dict(f.split("=") for f in line.split()[1:]) for line in out.splitlines() if line.startswith("case ")]
    assert len(rows) == len(cases)
    forms = set()
    for row, (m, ntab, nops, npairs, K, B, waves, cap, cus) in zip(rows, cases):
        want = sp.plan(m, ntab, nops, npairs, K, B, waves, cap, cus)
        assert int(row["fits"]) == int(sp.fits(m, ntab, K)) and int(row["ok"]) == int(want is not None), (row, want)
        if want is None:
            continue
        got = dict(nw=int(row["nw"]), stage=bool(int(row["stage"])), per_cu=int(row["per_cu"]), lds=int(row["lds"]), workgroups=int(row["workgroups"]))
        assert got == want, (row, want)
        forms.add((got["nw"], got["stage"]))
    assert forms == {(nw, stage) for nw in gc.WAVES for stage in (True, False)}, forms   # every instance of the kernel is planned somewhere


# ---- the closure rule --------------------------------------------------------------------------------------------------------------------
def _closure_by_the_header(check_program, tmp_path, case, support):
    f = tmp_path / "closure.txt"
    hx, hz, hc, _ = case.h
    f.write_text(f"{len(support)} {len(hc)}\n" + " ".join(str(int(a)) for a in support) + "\n" +
                 "".join(f"{int(x)} {int(z)} {float(c)!r}\n" for x, z, c in zip(hx, hz, hc)))
    row = dict(f.split("=") for f in check_program("--closure", f).split()[1:])
    return bool(int(row["odd_y"])), bool(int(row["leak"]))


@pytest.mark.parametrize("symbol, m", [("H2", 16), ("H4", 36), ("LiH", 225), ("H2O", 441)])
def test_molecular_supports_are_closed(check_program, tmp_path, symbol, m):
    """the UCCSD supports are closed under the molecular Hamiltonian, with residues above zero and below tiny = 64 eps sum |c|: a test
    for != 0.0 would send them to the streaming path"""
    case = sp.molecule(symbol)
    S = support_closure(case.hf, case.rx, case.rz, case.rc, case.pidx)
    odd_y, leak, worst = sp.exactness(case.h[0], case.h[1], case.h[2], S)
    print(f"{symbol}: support {S.size}, worst residue {worst:.3f} tiny")
    assert S.size == m and not odd_y and not leak and worst <= 1.0
    assert _closure_by_the_header(check_program, tmp_path, case, S) == (False, False)


def test_constructed_hamiltonians_are_not_closed(check_program, tmp_path):
    """per_rotation(3): the support is index bits 0 to 2; its own Hamiltonian is closed, + 0.3 X_5 leaks, + 0.2 Y_1 has an odd Y; the
    checker's S of the leaky one exceeds the closed one's by 0.09"""
    closed, leaky = sp.leak_case()
    _, oddy = sp.odd_y_case()
    S = support_closure(closed.hf, closed.rx, closed.rz, closed.rc, closed.pidx)
    assert S.tolist() == list(range(8))
    for case, want in ((closed, (False, False)), (leaky, (False, True)), (oddy, (True, False))):
        assert sp.case_exactness(case)[:2] == want and _closure_by_the_header(check_program, tmp_path, case, S) == want
    theta = np.random.default_rng(5).uniform(-0.6, 0.6, closed.K)
    for omega in (None, 0.4):
        s0, s1, s2 = (sp.case_want(c, theta, omega)[3] for c in (closed, leaky, oddy))
        assert abs(s1 - s0 - sp.LEAK_COEFF ** 2) <= 1e-13 and s2 - s0 > 1e-3
    # ... and the energies do not see either term: exactly why the compact program may drop them for <H>
    assert abs(leaky.want(theta)[0] - closed.want(theta)[0]) <= 1e-14 and abs(oddy.want(theta)[0] - closed.want(theta)[0]) <= 1e-14


# ---- surface -----------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_everywhere():
    from openvqe_amd import _lib, excited
    header = open(os.path.join(ROOT, "include", "ovqe_sv.h")).read()
    cdef = open(os.path.join(ROOT, "include", "ovqe_sv.cdef.h")).read()
    for name in ("ovqe_spread_gradient_batch", "ovqe_spread_info"):
        assert name + "(" in header and name + "(" in cdef and name in _lib.SIGNATURES
    assert "a spread Hessian" in header and "odd number of Y" in header and "64 eps" in header
    from openvqe_amd.backend import Statevector
    from openvqe_amd.partitioned import PartitionedStatevector
    for m in ("spread_gradient_batch", "energy_variance", "spread_info"):
        assert callable(getattr(Statevector, m))
        with pytest.raises(NotImplementedError):
            getattr(PartitionedStatevector, m)(None)
    assert callable(excited.folded_spectrum)


# ---- folded spectrum on the stand-in -----------------------------------------------------------------------------------------------------
def _h2_stand_in(h2):
    sv = sp.SpreadOracle(h2.n)
    sv.set_hamiltonian(h2.ham)
    sv.set_ucc_program(h2.gens, h2.hf)
    return sv


@pytest.fixture(scope="module")
def h2_levels(h2):
    from oracle import dense
    return np.linalg.eigvalsh(dense.operator_matrix(h2.ham, sparse=False))


def test_folded_spectrum_reaches_the_ground_state_of_h2(h2, h2_levels):
    """omega = E_0 + 0.02, start 0 at theta = 0: the nearest state the ansatz holds is the ground state itself — variance <= 1e-10,
    energy within 1e-6 of the dense ground value, spread (0.02)^2 to 1e-8"""
    from openvqe_amd import excited
    sv = _h2_stand_in(h2)
    e0 = float(h2_levels[0])
    (state,) = excited.folded_spectrum(sv, [e0 + 0.02], starts=1)
    print(f"H2: E_0 {e0:.10f}; energy {state['energy']:.10f} spread {state['spread']:.3e} variance {state['variance']:.3e} "
          f"iterations {state['result'].nit}")
    assert sv.spread_info()["mode"] == 1 and state["result"].best == 0 and state["theta"].shape == (h2.K,)
    assert state["variance"] <= 1e-10 and abs(state["energy"] - e0) <= 1e-6 and abs(state["spread"] - 0.02 ** 2) <= 1e-8
    assert np.all(np.diff(state["result"].energies) <= 0.0)
    assert abs(state["spread"] - state["variance"] - (state["energy"] - (e0 + 0.02)) ** 2) <= 1e-10
    e, var = sv.energy_variance(state["theta"])
    assert (e, var) == (state["energy"], state["variance"])
    with pytest.raises(ValueError):
        excited.folded_spectrum(sv, [e0], x0=np.zeros(h2.K + 1))
    with pytest.raises(ValueError):
        excited.folded_spectrum(sv, [e0], starts=0)


def test_folded_spectrum_near_higher_levels_of_h2(h2, h2_levels):
    """omega near higher eigenvalues: the ansatz need not hold an eigenstate there, so only what is rigorous — an eigenvalue of H on the
    register lies within sqrt(variance) of every returned energy (Weinstein), and no state has a spread below min_k (E_k - omega)^2"""
    from openvqe_amd import excited
    sv = _h2_stand_in(h2)
    omegas = [float(h2_levels[k]) + 0.01 for k in (1, 5, 20)] + [float(h2_levels[0]) - 0.5]
    states = excited.folded_spectrum(sv, omegas, starts=3, spread=0.3, seed=1, maxiter=150)
    assert len(states) == len(omegas)
    for omega, s in zip(omegas, states):
        nearest = float(np.abs(h2_levels - s["energy"]).min())
        print(f"omega {omega:.6f}: energy {s['energy']:.8f} spread {s['spread']:.3e} variance {s['variance']:.3e} nearest level at {nearest:.3e}")
        assert nearest <= np.sqrt(s["variance"]) + 1e-9
        assert s["spread"] >= float(((h2_levels - omega) ** 2).min()) - 1e-9
        assert s["variance"] >= -1e-12 and s["spread"] >= s["variance"] - 1e-9
