"""CPU tests of the batched exact gradient's infrastructure (tests/gradbatch_cases.py): the checker against central differences of the
oracle's energies, the restated LDS formula and planner rule against the host-only planner (openvqe_amd/csrc/sv_gradbatch_host.hpp)
replayed by tests/cpu/gradbatch_plan_check.cpp under ASan + UBSan with g++ alone, the declared surface, and the Python layers on a
stand-in backend."""
import os
import subprocess

import numpy as np
import pytest

from oracle import masks
from tests import gradbatch_cases as gc
from tests.oracle_backend import OracleStatevector

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_checker_against_central_differences():
    """``masks.ucc_energy_gradient`` on the cases the GPU tests use at the support edges against central differences (step 1e-5) of the
    oracle's energy: 1e-8 ||H||_1 max(1, C) — truncation h^2 C^3 / 6 ~ 2e-11 and rounding eps / h ~ 2e-11, two orders of margin"""
    for what, case in (("two states", gc.two_states()[0]), ("no active op", gc.no_active_op()[0]), ("y program", gc.y_program(14))):
        theta = np.random.default_rng(5).uniform(-0.8, 0.8, case.K)
        e, g = case.want(theta)
        h = 1e-5
        for k in range(case.K):
            d = np.eye(case.K)[k] * h
            ep = masks.ucc_energy_gradient(case.n, case.hf, case.rx, case.rz, case.rc, case.pidx, theta + d, *case.h)[0]
            em = masks.ucc_energy_gradient(case.n, case.hf, case.rx, case.rz, case.rc, case.pidx, theta - d, *case.h)[0]
            assert abs((ep - em) / (2 * h) - g[k]) <= 1e-8 * case.h1 * max(1.0, case.C), (what, k)
        if what == "no active op":
            assert g[0] == 0.0
        else:
            assert np.abs(g).max() > 1e-3


def test_lds_formula_restated():
    """H2O-like sizes by hand, and the decisions at m = 4096"""
    assert gc.wave_stride(441, 1000, 140) == 2 * 442 * 8 + 24000 + 1120
    assert gc.wave_stride(225, 7, 3) == (2 * 226 * 8 + 168 + 32 + 15) // 16 * 16
    assert gc.batch_lds_bytes(441, 1000, 300, 5000, 140, 4, True) == 4 * gc.wave_stride(441, 1000, 140) + 4800 + 20000
    assert gc.batch_lds_bytes(441, 1000, 300, 5000, 140, 4, False) == 4 * gc.wave_stride(441, 1000, 140)
    b = gc.y_boundaries()
    print(b)
    # two regions of 64 KiB + tables leave 21 KiB: the 4095 pair words of the first twelve rotations fit, 2048 more do not
    assert (b["two_staged"], b["two_plain"]) == (12, 13)
    # 24 bytes of table per rotation: two regions up to 75 KiB each, one up to 150 KiB
    assert (b["two_last"], b["one_first"]) == (461, 462) and (b["path1_last"], b["path2_first"]) == (3661, 3662)
    for R, waves, nw, form in gc.y_boundary_cases():
        p = gc.plan(*gc.y_sizes(R), 3, waves=waves)
        assert (p is None and form == 0) or ((p["nw"], 1 if p["stage"] else 2) == (nw, form) and p["lds"] <= gc.LDS_BUDGET), (R, waves, p)
    assert gc.plan(*gc.y_sizes(b["path1_last"]), 3)["lds"] + 24 > gc.LDS_BUDGET
    # the rule on a small program (one region 5168 bytes, tables 4400): the registers bound every geometry, 24 waves are the most
    # (one wave staged: 17 workgroups; two: 11 x 2; four: 6 x 4 = 24; unstaged: 24 x 1) and the first in the order of the ties has them
    small = gc.plan(70, 160, 100, 700, 26, 4096)
    assert gc.wave_stride(70, 160, 26) == 5168
    assert (small["nw"], small["stage"], small["per_cu"], small["lds"]) == (4, True, 6, 4 * 5168 + 4400) and small["workgroups"] == 1024
    assert gc.plan(70, 160, 100, 700, 26, 4096, cus=4)["workgroups"] == 24 and gc.plan(70, 160, 100, 700, 26, 9, workgroups=2)["workgroups"] == 2
    assert gc.plan(70, 160, 100, 700, 26, 3, waves=8)["workgroups"] == 1


def _planner_cases():
    b = gc.y_boundaries()
    cases = []
    for R, waves, _, _ in gc.y_boundary_cases():   # the boundaries at m = 4096
        cases.append(gc.y_sizes(R) + (3, waves, 0, 256))
    lih, h2o = (225, 1100, 700, 6000, 92), (441, 2500, 1500, 20000, 140)   # sizes of the kind the molecules have
    for sizes in (lih, h2o, (70, 160, 100, 700, 26), (1, 2, 0, 0, 1), (2, 1, 1, 1, 1)):
        for B in (1, 3, 64, 4096):
            cases.append(sizes + (B, 0, 0, 256))
        for nw in gc.WAVES:
            for B in (1, nw - 1, nw, nw + 1, 5 * nw + 1):   # B < nw: waves without a row
                if B >= 1:
                    cases.append(sizes + (B, nw, 0, 256))
            cases.append(sizes + (5 * nw + 1, nw, 2, 256))
        cases.append(sizes + (100000, 0, 0, 8))
        cases.append(sizes + (7, 3, 0, 256))   # an option value that is no wave count: automatic
    rng = np.random.default_rng(11)
    for _ in range(200):
        m = int(rng.integers(1, 4097))
        cases.append((m, int(rng.integers(1, 5000)), int(rng.integers(0, 3000)), int(rng.integers(0, 40000)), int(rng.integers(1, 300)),
                      int(rng.integers(1, 5000)), int(rng.choice([0, 0, 1, 2, 4, 8])), int(rng.choice([0, 0, 1, 7, 300])),
                      int(rng.choice([1, 8, 256, 304]))))
    return cases


def test_planner_under_asan_ubsan(tmp_path):
    src = os.path.join(ROOT, "tests", "cpu", "gradbatch_plan_check.cpp")
    exe = str(tmp_path / "gradbatch_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-o", exe, src])
    cases = _planner_cases()
    listing = tmp_path / "cases.txt"
    listing.write_text("".join(" ".join(str(v) for v in c) + "\n" for c in cases))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, str(listing)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert f"gradbatch plan ok ({len(cases)} cases)" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    rows = [dict(f.split("=") for f in line.split()[1:]) for line in r.stdout.splitlines() if line.startswith("case ")]
    assert len(rows) == len(cases)
    forms = set()
    for row, (m, ntab, nops, npairs, K, B, waves, cap, cus) in zip(rows, cases):
        want = gc.plan(m, ntab, nops, npairs, K, B, waves, cap, cus)
        assert int(row["eligible"]) == int(gc.eligible(m, ntab, K)), row
        assert int(row["ok"]) == int(want is not None), (row, want)
        if want is None:
            continue
        got = dict(nw=int(row["nw"]), stage=bool(int(row["stage"])), per_cu=int(row["per_cu"]), lds=int(row["lds"]),
                   workgroups=int(row["workgroups"]))
        assert got == want, (row, want)
        forms.add((got["nw"], got["stage"]))
    assert forms == {(nw, stage) for nw in gc.WAVES for stage in (True, False)}, forms   # every instance of the kernel is planned somewhere


def test_symbols_are_declared_everywhere():
    from openvqe_amd import _lib
    header = open(os.path.join(ROOT, "include", "ovqe_sv.h")).read()
    cdef = open(os.path.join(ROOT, "include", "ovqe_sv.cdef.h")).read()
    for name in ("ovqe_energy_gradient_batch", "ovqe_gradient_batch_info"):
        assert name + "(" in header and name + "(" in cdef and name in _lib.SIGNATURES
    assert "grad_batch_waves" in header and "grad_batch_workgroups" in header
    assert "Out of scope: batched forms of the sector and the streaming paths" in header
    from openvqe_amd.backend import Statevector
    from openvqe_amd.evaluator import _Evaluator
    from openvqe_amd.partitioned import PartitionedStatevector
    from openvqe_amd.ucc_family.get_energy_ucc import EnergyUCC
    for m in ("energy_gradient_batch", "gradient_batch_info"):
        assert callable(getattr(Statevector, m))
    assert callable(_Evaluator.energy_gradient_batch) and callable(PartitionedStatevector.energy_gradient_batch)
    assert EnergyUCC.multistart == 0 and EnergyUCC.multistart_spread == 0.1 and EnergyUCC.multistart_seed == 0


class BatchOracle(OracleStatevector):
    """the stand-in backend with the batched call, from the checker"""

    def energy_gradient_batch(self, thetas):
        thetas = np.ascontiguousarray(thetas, np.float64)
        if thetas.ndim != 2 or thetas.shape[1] != self._K:
            raise ValueError("shape")
        _, xs, zs, cs, p0, pi, hf = self._prog
        hx, hz, hc, const = self._ham
        out = [masks.ucc_energy_gradient(self.nbqbits, hf, xs, zs, cs, pi, t, hx, hz, hc, const, p0) for t in thetas]
        return np.array([e for e, _ in out]), np.array([g for _, g in out]).reshape(len(out), thetas.shape[1])


def test_multistart_vqe_through_the_mirror_on_the_oracle(monkeypatch):
    """EnergyUCC.multistart on H2/STO-3G with the stand-in backend: the ground energy from four starts, the accepted energies appended to
    ``energies``, the options that do not combine refused, and the defaults untouched"""
    import json

    from openvqe_amd import evaluator, fermion
    from openvqe_amd.operators import Hamiltonian, Term
    from openvqe_amd.ucc_family.get_energy_ucc import EnergyUCC
    k1 = json.load(open(os.path.join(ROOT, "tests", "golden", "k1_h2_sto3g.json")))
    H = Hamiltonian(4, [Term(c, o, q) for c, o, q in k1["terms"]], k1["constant_coeff"])
    gens = fermion.uccsd_generators(2, 1)
    monkeypatch.setattr(evaluator, "shared_backend", lambda n, device=None: BatchOracle(n))
    monkeypatch.setattr(evaluator._Evaluator, "_owner", {})

    class Multi(EnergyUCC):
        multistart = 4
        multistart_spread = 0.2

    energies = []
    res = Multi()._minimize(H, gens, k1["hf_init"], np.zeros(3), energies, "BFGS", 1e-7)
    print(res.message, res.nit, res.ncalls, res.rows, res.fun, res.F)
    assert res.success and res.converged.all() and np.abs(res.G[res.converged]).max() <= 1e-7
    assert np.ptp(res.F) < 1e-10 and energies == res.energies and np.all(np.diff(energies) <= 0.0)
    assert res.X.shape == (4, 3) and res.rows < res.ncalls * 4 + 4
    single = EnergyUCC()
    single.adjoint_gradient = True
    ref = single._minimize(H, gens, k1["hf_init"], np.zeros(3), [], "BFGS", 1e-7)
    assert abs(res.fun - ref.fun) < 1e-9

    class Both(Multi):
        newton = True

    with pytest.raises(ValueError):
        Both()._minimize(H, gens, k1["hf_init"], np.zeros(3), [], "BFGS", 1e-7)
    Both.newton, Both.natural_gradient = False, True
    with pytest.raises(ValueError):
        Both()._minimize(H, gens, k1["hf_init"], np.zeros(3), [], "BFGS", 1e-7)
