"""CPU tests of finite-shot measurement: the checker (tests/measure_cases.py) on itself, the host restatement of the uniforms
(openvqe_amd/synth.py), the grouping planner (openvqe_amd/csrc/sv_measure_host.hpp) replayed by tests/cpu/measure_plan_check.cpp under
ASan + UBSan with g++ alone and compared with the Python restatement, the declared surface, and the nbshots logic of the qat stand-ins
on a numpy backend that implements the contract of include/ovqe_sv.h."""
import json
import os
import subprocess

import numpy as np
import pytest

from openvqe_amd import fermion, synth
from openvqe_amd.operators import Hamiltonian, Term, pack_terms
from tests import measure_cases as mc
from tests.oracle_backend import OracleStatevector

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _k1():
    k1 = json.load(open(os.path.join(ROOT, "tests", "golden", "k1_h2_sto3g.json")))
    return k1, Hamiltonian(4, [Term(c, o, q) for c, o, q in k1["terms"]], k1["constant_coeff"])


# ---- uniforms -----------------------------------------------------------------------------------------------------------------------
def test_shot_uniforms_are_chunk_invariant_and_match_the_integer_restatement():
    for seed, stream in ((0, 0), (7, 3), ((1 << 64) - 1, 1 << 63), (20250227, 141)):
        whole = synth.shot_uniforms(seed, stream, 0, 1000)
        assert whole.dtype == np.float64 and whole.shape == (1000,)
        assert whole.min() >= 0.0 and whole.max() < 1.0
        parts = np.concatenate([synth.shot_uniforms(seed, stream, a, b - a) for a, b in ((0, 1), (1, 64), (64, 65), (65, 700), (700, 1000))])
        assert np.array_equal(whole.view(np.int64), parts.view(np.int64))
        assert np.array_equal(whole, mc.uniforms(seed, stream, 0, 1000))
        assert np.array_equal(synth.shot_uniforms(seed, stream, (1 << 40) + 5, 9), mc.uniforms(seed, stream, (1 << 40) + 5, 9))
    a, b = synth.shot_uniforms(1, 0, 0, 4096), synth.shot_uniforms(1, 1, 0, 4096)
    assert not np.array_equal(a, b) and abs(a.mean() - 0.5) < 0.03 and abs(np.corrcoef(a, b)[0, 1]) < 0.06
    assert synth.shot_uniforms(3, 4, 10, 0).shape == (0,)


# ---- the checker on itself -----------------------------------------------------------------------------------------------------------
def test_basis_change_conventions():
    s = np.sqrt(0.5)
    plus_i, minus_i = np.array([s, 1j * s]), np.array([s, -1j * s])
    assert np.allclose(mc.probabilities(plus_i, 1, 0, 1), [1, 0]) and np.allclose(mc.probabilities(minus_i, 1, 0, 1), [0, 1])
    assert np.allclose(mc.probabilities(np.array([s, s]), 1, 1, 0), [1, 0]) and np.allclose(mc.probabilities(np.array([s, -s]), 1, 1, 0), [0, 1])
    # index bit b <-> qubit n - 1 - b: |+> on index bit 0 of three, |1> on bit 2
    psi = np.zeros(8, complex)
    psi[0b100], psi[0b101] = s, s
    assert np.allclose(mc.probabilities(psi, 3, 0b001, 0), np.eye(8)[0b100])
    # B is unitary: the weight is kept
    rng = np.random.default_rng(5)
    psi = rng.normal(size=64) + 1j * rng.normal(size=64)
    assert abs(mc.probabilities(psi, 6, 0b101001, 0b010010).sum() - np.vdot(psi, psi).real) < 1e-12


def test_exact_rule_and_acceptance_rule():
    p = np.array([0.0, 0.5, 0.0, 0.0, 1.5, 0.0])          # W = 2
    u = np.array([0.0, 0.2499999, 0.25, 0.9999999999, 0.6])
    want = [1, 1, 4, 4, 4]
    assert list(mc.exact_outcomes(p, u)) == want
    assert mc.check_outcomes(want, p, u, "exact") == 0
    with pytest.raises(AssertionError):
        mc.check_outcomes([1, 1, 3, 4, 4], p, u, "a zero-probability index")
    with pytest.raises(AssertionError):
        mc.check_outcomes([1, 4, 4, 4, 4], p, u, "outside the interval")
    # inside the margin: allowed, counted, capped at 1 %
    pm = np.full(1000, 1e-3)
    um = np.full(200, 0.5 + 1e-10)
    assert list(mc.exact_outcomes(pm, um[:1])) == [500]
    with pytest.raises(AssertionError):
        mc.check_outcomes([499] * 200, pm, um, "margin everywhere")
    um2 = np.concatenate([um[:1], np.full(199, 0.25005)])
    assert mc.check_outcomes([499] + [250] * 199, pm, um2, "one margin shot of 200") == 1


def test_margin_of_the_exact_rule_for_the_seeds_of_the_gpu_tests():
    """the share of shots within eps W of an interval boundary — the shots whose outcome a different summation order may change — stays
    far below the 1 % cap for the seeds, sizes and shot counts the GPU tests use (expected <= 2 eps N)"""
    for n, shots in ((10, 100000), (16, 100000), (20, 4096)):
        psi = synth.amplitudes(11 + n, np.arange(1 << n, dtype=np.uint64))
        p = psi.real ** 2 + psi.imag ** 2
        C = mc.exact_prefix(p)
        t = np.asarray(synth.shot_uniforms(100 + n, 0, 0, shots), np.longdouble) * C[-1]
        i = np.searchsorted(C, t, side="right")
        near = (np.abs(C[i] - t) <= mc.EPS * C[-1]) | (np.abs(t - np.where(i > 0, C[np.maximum(i - 1, 0)], 0)) <= mc.EPS * C[-1])
        print(n, shots, int(near.sum()))
        assert near.sum() <= 0.002 * shots + 2


def test_signs_and_scores():
    idx = np.array([0b0000, 0b0101, 0b1111, 0b1000], np.uint64)
    assert list(mc.signs(idx, 0b0101)) == [1, 1, 1, 1] and list(mc.signs(idx, 0b1100)) == [1, -1, 1, -1]
    tsum, v = mc.score(idx, [0b0001, 0b1000], [0.5, -2.0])
    assert list(tsum) == [0, 0] and np.allclose(v, [-1.5, -2.5, 1.5, 2.5])
    e, s = mc.estimate(0.5, 4, [v.sum()], [(v * v).sum()])
    assert abs(e - 0.5) < 1e-15 and abs(s - np.std(v, ddof=1) / 2) < 1e-15


# ---- planner -------------------------------------------------------------------------------------------------------------------------
def _random_terms(rng, n, T):
    xs = rng.integers(0, 1 << n, T, dtype=np.uint64)
    zs = rng.integers(0, 1 << n, T, dtype=np.uint64)
    sparse = rng.random(T) < 0.6          # low-weight strings make groups that actually merge
    keep = rng.integers(0, 1 << n, T, dtype=np.uint64) & rng.integers(0, 1 << n, T, dtype=np.uint64)
    xs = np.where(sparse, xs & keep, xs)
    zs = np.where(sparse, zs & keep, zs)
    cs = np.round(rng.normal(size=T), 1)   # ties in |coeff|: the stored position decides
    if T > 3:
        xs[T // 2] = zs[T // 2] = 0        # an identity term
    return xs, zs, cs


def test_python_planner_on_k1_gives_five_groups():
    k1, H = _k1()
    xs, zs, cs = pack_terms(4, H.terms)
    group, xb, yb = mc.plan_groups(xs, zs, cs.real)
    mc.check_plan(4, xs, zs, cs.real, group, xb, yb)
    assert len(xb) == 5
    diag = {t for t in range(len(xs)) if not int(xs[t])}
    assert {t for t in range(len(xs)) if group[t] == 0} == diag and int(xb[0]) == 0 and int(yb[0]) == 0
    names = [k1["terms"][t][1] for t in range(len(xs)) if t not in diag]
    assert sorted(names) == ["XXYY", "XYYX", "YXXY", "YYXX"]
    assert sorted(int(group[t]) for t in range(len(xs)) if t not in diag) == [1, 2, 3, 4]


def test_measure_plan_under_asan_ubsan(tmp_path):
    rng = np.random.default_rng(2025)
    cases = []
    _, H = _k1()
    xs, zs, cs = pack_terms(4, H.terms)
    cases.append((4, xs, zs, cs.real))
    for n in (1, 2, 3, 5, 8, 10):
        for T in (0, 1, 7, 60):
            cases.append((n,) + _random_terms(rng, n, T))
    path = tmp_path / "cases.txt"
    with open(path, "w") as f:
        for n, xs, zs, cs in cases:
            f.write(f"{n} {len(xs)}\n")
            for x, z, c in zip(xs, zs, cs):
                f.write(f"{int(x):x} {int(z):x} {float(c).hex()}\n")
    src = os.path.join(ROOT, "tests", "cpu", "measure_plan_check.cpp")
    exe = str(tmp_path / "measure_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-o", exe, src])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, str(path)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert f"measure plan ok: {len(cases)} cases" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    lines = r.stdout.splitlines()
    at = 0
    for k, (n, xs, zs, cs) in enumerate(cases):
        group, xb, yb = mc.plan_groups(xs, zs, cs)
        mc.check_plan(n, xs, zs, cs, group, xb, yb)
        assert lines[at] == f"case {len(xb)}", (k, lines[at])
        assert [int(v) for v in lines[at + 1].split()] == [int(g) for g in group], k
        for g in range(len(xb)):
            assert lines[at + 2 + g] == f"{int(xb[g]):x} {int(yb[g]):x}", (k, g)
        at += 2 + len(xb)
        if k == 0:
            assert len(xb) == 5      # K1: the diagonal terms, XXYY, YYXX, XYYX, YXXY


# ---- declared surface ----------------------------------------------------------------------------------------------------------------
def test_measure_symbols_are_declared_everywhere():
    from openvqe_amd import _lib
    header = open(os.path.join(ROOT, "include", "ovqe_sv.h")).read()
    cdef = open(os.path.join(ROOT, "include", "ovqe_sv.cdef.h")).read()
    for name in ("ovqe_sample", "ovqe_measure_paulis", "ovqe_measure_groups", "ovqe_energy_sampled", "ovqe_measure_info"):
        assert name + "(" in header and name + "(" in cdef and name in _lib.SIGNATURES
    from openvqe_amd.backend import Statevector
    from openvqe_amd.partitioned import PartitionedStatevector
    for m in ("sample", "measure_paulis", "measurement_groups", "energy_sampled", "measure_info"):
        assert callable(getattr(Statevector, m))
    for m in ("sample", "energy_sampled"):
        with pytest.raises(NotImplementedError, match="partitioned register"):
            getattr(PartitionedStatevector, m)(None)


# ---- the qat stand-ins on a numpy backend that implements the contract ---------------------------------------------------------------
class SamplingOracle(OracleStatevector):
    """the stand-in backend with the measuring calls, by the exact rule of the checker"""

    def sample(self, n_shots, seed=0, stream=0, first_shot=0):
        p = mc.probabilities(self.psi, self.nbqbits)
        return mc.exact_outcomes(p, synth.shot_uniforms(seed, stream, first_shot, n_shots))

    def measurement_groups(self):
        xs, zs, cs, _ = self._ham
        return mc.plan_groups(xs, zs, cs)

    def energy_sampled(self, theta, n_shots, seed=0):
        if n_shots < 2:
            raise ValueError("n_shots < 2")
        self.prepare_state(theta)
        xs, zs, cs, const = self._ham
        e, s, *_ = mc.replay_energy(self.psi, self.nbqbits, xs, zs, cs, const, self.measurement_groups(), n_shots, seed)
        return e, s


@pytest.fixture()
def sampling_engine(monkeypatch):
    import openvqe_amd.backend as be
    import openvqe_amd.qat_compat as qc
    monkeypatch.setattr(be, "Statevector", SamplingOracle)
    monkeypatch.setattr(qc, "_default_qpu", None)
    yield qc
    qc._default_qpu = None


def _h2_circuit(qc, theta):
    k1, H = _k1()
    gens = fermion.uccsd_generators(2, 1)
    prog = qc.Program()
    reg = prog.qalloc(4)
    prog.apply(qc.build_ucc_ansatz(gens, k1["hf_init"])(list(theta)), reg)
    return prog.to_circ(), H


def test_hipqpu_with_and_without_shots(sampling_engine):
    qc = sampling_engine
    theta = [0.05, -0.03, -0.1137]
    circ, H = _h2_circuit(qc, theta)
    # nbshots = 0: today's answers, whatever the seed
    exact = qc.HipQPU().submit(circ.to_job(job_type="OBS", observable=H)).value
    sv = OracleStatevector(4)
    sv.set_hamiltonian(H)
    sv.set_ucc_program(fermion.uccsd_generators(2, 1), 12)
    assert exact == sv.energy(theta)
    job0 = circ.to_job(job_type="OBS", observable=H, nbshots=0)
    assert job0.nbshots == 0 and circ.to_job().nbshots == 0 and circ.to_job(nbshots=77).nbshots == 77
    r0 = qc.HipQPU(seed=5).submit(job0)
    assert r0.value == exact and r0.error is None
    amps = {s.state.int: s.amplitude for s in qc.HipQPU(seed=9).submit(circ.to_job())}
    assert amps and all(a is not None for a in amps.values()) and abs(sum(abs(a) ** 2 for a in amps.values()) - 1) < 1e-12
    # OBS with shots: an estimate with its standard error; the same seed repeats it, the next submission does not
    a, b = qc.HipQPU(seed=3), qc.HipQPU(seed=3)
    job = circ.to_job(job_type="OBS", observable=H, nbshots=2048)
    ra1, ra2, rb1 = a.submit(job), a.submit(job), b.submit(job)
    assert ra1.value == rb1.value and ra1.error == rb1.error and ra1.value != ra2.value
    assert 0 < ra1.error < 0.02 and abs(ra1.value - exact) < 5 * ra1.error and abs(ra2.value - exact) < 5 * ra2.error
    assert qc.HipQPU(seed=4).submit(job).value != ra1.value
    assert a.submissions == 2
    # SAMPLE with shots: frequencies in ascending state order
    res = a.submit(circ.to_job(nbshots=1000))
    states = [s.state.int for s in res]
    assert states == sorted(states) and len(set(states)) == len(states) and set(states) <= set(amps)
    assert all(s.amplitude is None for s in res) and abs(sum(s.probability for s in res) - 1.0) < 1e-12
    assert all(round(s.probability * 1000) == s.probability * 1000 for s in res)
    top = max(res, key=lambda s: s.probability)
    assert top.state.int == 12 and abs(top.probability - abs(amps[12]) ** 2) < 0.05
    with pytest.raises(ValueError):
        circ.to_job(nbshots=-1)


def test_partitioned_register_names_the_limit(sampling_engine, monkeypatch):
    qc = sampling_engine
    from openvqe_amd import partitioned

    class Refusing(SamplingOracle):
        sample = energy_sampled = partitioned.PartitionedStatevector.sample

    import openvqe_amd.backend as be
    monkeypatch.setattr(be, "Statevector", Refusing)
    circ, H = _h2_circuit(qc, [0.1, 0.2, 0.3])
    qpu = qc.HipQPU()
    assert qpu.submit(circ.to_job(job_type="OBS", observable=H)).value < 0       # nbshots = 0 still runs
    with pytest.raises(NotImplementedError, match="partitioned register"):
        qpu.submit(circ.to_job(job_type="OBS", observable=H, nbshots=100))
    with pytest.raises(NotImplementedError, match="partitioned register"):
        qpu.submit(circ.to_job(nbshots=100))
