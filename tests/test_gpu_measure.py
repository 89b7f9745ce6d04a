"""GPU tests of finite-shot measurement (ovqe_sample, ovqe_measure_paulis, ovqe_measure_groups, ovqe_energy_sampled,
ovqe_measure_info: csrc/sv_measure_host.hpp, sv_measure.hpp, measure_host.inc; Statevector.sample / measure_paulis /
measurement_groups / energy_sampled / measure_info; the nbshots path of the qat stand-ins) against the checker of tests/measure_cases.py.

Every outcome must pass the checker's acceptance rule (p_i > 0 and C_{i-1} - eps W <= u W <= C_i + eps W with exact C, eps = 1e-9), at
most 1 % of a test's shots may differ from the exact rule's outcome.  Sizes: 1 and 2 qubits (less than a wave of amplitudes), 6 and 7
(one wave / two), 10 and 11 (below / at one scan chunk and one LDS tile of 2048), 12, 13 and 16 (several chunks; rotated bits above the
tile from 12 on), 20 (512 chunk totals: the totals scan walks more than one step of 256)."""
import re

import numpy as np
import pytest

from openvqe_amd import synth
from tests import measure_cases as mc

pytestmark = pytest.mark.gpu

INVALID, STATE = -1, -5


@pytest.fixture(scope="module")
def SV(gpu_lib):
    from openvqe_amd.backend import Statevector
    return Statevector


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _code(call):
    """-> (error code, text) of a refused call"""
    from openvqe_amd import _lib
    with pytest.raises(_lib.BackendError) as ei:
        call()
    m = re.match(r"libovqe_sv error (-?\d+): (.*)", str(ei.value), flags=re.S)
    return int(m.group(1)), m.group(2)


def _p(psi):
    return psi.real ** 2 + psi.imag ** 2


# ---- sampling ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 6, 7, 10, 11, 12, 13, 16, 20])
def test_sampling(SV, n):
    big = 4096 if n == 20 else 100000
    N = 1 << n
    with SV(n) as sv:
        states = dict(mc.spike_states(n))
        sv.randomize(11 + n)
        states["randomized"] = sv.get_state()
        for name, psi in states.items():
            what = f"n {n} {name}"
            sv.set_state(psi)
            before = sv.get_state()
            seed = 100 + n
            whole = sv.sample(big, seed=seed)
            info = sv.measure_info()
            assert whole.dtype == np.uint64 and whole.shape == (big,)
            assert info["groups"] == 1 and info["shots"] == big and info["high_passes"] == 0 and info["scratch_bytes"] >= 8 * N, info
            p = _p(psi)
            mc.check_outcomes(whole, p, synth.shot_uniforms(seed, 0, 0, big), what)
            if name in ("first", "last"):
                assert np.all(whole == (0 if name == "first" else N - 1)), what
            if name == "two spikes":
                assert set(np.unique(whole)) == {0, N - 1} and abs(np.mean(whole == 0) - p[0] / p.sum()) < 0.03, what
            # the small counts are the first shots of the large draw; pieces are the whole; a second call repeats the bits
            for k in (0, 1, 63, 64, 65):
                part = sv.sample(k, seed=seed)
                assert part.shape == (k,) and np.array_equal(part, whole[:k]), (what, k)
            pieces = np.concatenate([sv.sample(b - a, seed=seed, first_shot=a) for a, b in ((0, 1), (1, 65), (65, 1000), (1000, 4096))])
            assert np.array_equal(pieces, whole[:4096]), what
            assert np.array_equal(sv.sample(big, seed=seed), whole), what
            if name in ("randomized", "two spikes"):
                other = sv.sample(4096, seed=seed + 1)
                assert not np.array_equal(other, whole[:4096]), what
                assert not np.array_equal(sv.sample(4096, seed=seed, stream=1), whole[:4096]), what
                mc.check_outcomes(sv.sample(4096, seed=seed, stream=5, first_shot=1 << 40), p, synth.shot_uniforms(seed, 5, 1 << 40, 4096), what + " stream 5")
            assert np.array_equal(_bits(sv.get_state()), _bits(before)), what       # psi is only read


def test_sparse_lih_state_never_returns_a_zero_probability_index(SV):
    """LiH/STO-3G UCCSD, 12 qubits: the streamed state carries 225 amplitudes of weight, rounding dust (1e-37 and below) on the rest of
    its symmetry sector, and exact zeros — three quarters of the register — everywhere else, in runs between the sector's indices"""
    c = mc.energy_case("LiH")
    with SV(c.n) as sv:
        c.load(sv)
        sv.prepare_state(c.theta)
        psi = sv.get_state()
        p = _p(psi)
        assert c.n == 12 and 225 <= np.count_nonzero(p) <= 1024 and np.count_nonzero(p > 1e-30) <= 225
        idx = sv.sample(100000, seed=77)
        assert np.all(p[idx.astype(np.int64)] > 0)
        mc.check_outcomes(idx, p, synth.shot_uniforms(77, 0, 0, 100000), "LiH")
        assert np.array_equal(_bits(sv.get_state()), _bits(psi))


# ---- basis change ----------------------------------------------------------------------------------------------------------------------
def _masks(n):
    """(xbasis, ybasis): no bit, the lowest, the highest, all bits — x only, y only, mixed — and masks that straddle the 2^11 tile"""
    top, every = 1 << (n - 1), (1 << n) - 1
    alt = int("01" * 32, 2) & every
    out = [(0, 0), (1, 0), (0, 1), (top, 0), (0, top), (every, 0), (0, every), (alt, every & ~alt)]
    if n >= 2:
        out += [(1, top), (top, 1)]
    if n >= 13:
        out += [(0b11 << 10, 0), (0, 0b11 << 10), (1 << 10 | 1 << (n - 1), 1 << 11 | 1), (0b1001 << 9, 0b0110 << 9)]
    return out


@pytest.mark.parametrize("n", [1, 2, 6, 11, 13, 14, 15, 16])
def test_basis_change_and_scores(SV, n):
    shots = 20000
    rng = np.random.default_rng(n)
    every = (1 << n) - 1
    with SV(n) as sv:
        sv.randomize(500 + n)
        psi = sv.get_state()
        for k, (xb, yb) in enumerate(_masks(n)):
            what = f"n {n} xbasis {xb:#x} ybasis {yb:#x}"
            T = 1 + k % 5
            tm = rng.integers(1, every + 1, T, dtype=np.uint64)
            tc = rng.normal(size=T)
            tsum, vsum, idx = sv.measure_paulis(tm, tc, shots, xbasis=xb, ybasis=yb, seed=9 + k, stream=k, return_indices=True)
            info = sv.measure_info()
            high = bin((xb | yb) >> 11).count("1")
            assert info["high_passes"] == high and info["terms"] == T and info["scratch_bytes"] >= (8 << n) + ((16 << n) if high else 0), (what, info)
            mc.check_outcomes(idx, mc.probabilities(psi, n, xb, yb), synth.shot_uniforms(9 + k, k, 0, shots), what)
            want_t, vals = mc.score(idx, tm, tc)
            assert tsum.dtype == np.int64 and np.array_equal(tsum, want_t), what          # integers: exact
            # sums of `shots` values of magnitude |v_s| in any order: within shots 2^-53 sum |v_s| — 1e-12 relative to the absolute sums
            assert abs(vsum[0] - vals.sum()) <= 1e-12 * np.abs(vals).sum(), (what, vsum, vals.sum())
            assert abs(vsum[1] - (vals * vals).sum()) <= 1e-12 * (vals * vals).sum(), what
            again = sv.measure_paulis(tm, tc, shots, xbasis=xb, ybasis=yb, seed=9 + k, stream=k)
            assert np.array_equal(again[0], tsum) and np.array_equal(_bits(again[1]), _bits(vsum)), what   # without indices, bit for bit
            assert np.array_equal(_bits(sv.get_state()), _bits(psi)), what
        # no basis change and no term is sample()
        assert np.array_equal(sv.measure_paulis([], [], 1000, seed=3, return_indices=True)[2], sv.sample(1000, seed=3))


@pytest.mark.parametrize("n", [1, 5, 13, 16])
def test_eigenstates_pin_the_conventions(SV, n):
    N, every = 1 << n, (1 << n) - 1
    with SV(n) as sv:
        sv.set_state(np.full(N, 1.0 / np.sqrt(N)))                       # |+>^n in X: all zeros
        tsum, vsum, idx = sv.measure_paulis([every, 1], [1.0, 0.5], 5000, xbasis=every, return_indices=True)
        assert not idx.any() and list(tsum) == [5000, 5000] and vsum[0] == 7500.0 and vsum[1] == 5000 * 2.25
        for b in sorted({0, n - 1, min(n - 1, 11), min(n - 1, 10)}):    # both Y eigenstates on one bit, |0> elsewhere
            for sign in (1, -1):
                psi = np.zeros(N, complex)
                psi[0], psi[1 << b] = np.sqrt(0.5), sign * 1j * np.sqrt(0.5)
                sv.set_state(psi)
                idx = sv.measure_paulis([], [], 3000, ybasis=1 << b, seed=b, return_indices=True)[2]
                assert np.all(idx == (0 if sign > 0 else 1 << b)), (n, b, sign)      # (|0> + i|1>)/sqrt 2 gives bit 0
                idx = sv.measure_paulis([], [], 3000, xbasis=1 << b, seed=b, return_indices=True)[2]   # in X: both outcomes
                assert set(np.unique(idx)) == {0, 1 << b}
        psi = np.zeros(N, complex)                                       # |-> on the highest bit: eigenvalue -1 <-> bit 1
        psi[0], psi[N >> 1] = np.sqrt(0.5), -np.sqrt(0.5)
        sv.set_state(psi)
        tsum, _, idx = sv.measure_paulis([N >> 1], [1.0], 100, xbasis=N >> 1, return_indices=True)
        assert np.all(idx == N >> 1) and list(tsum) == [-100]


# ---- energies with shot noise ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["H2", "LiH", "random8"])
def test_energy_sampled_by_replay(SV, name):
    """n_shots = 4096 per group.  The seeds were picked on the CPU so that the replayed estimate lies within 3 exact standard
    deviations of the exact energy: H2 (seed 1) replay -1.102842 against -1.100419, sd 0.002506 (-0.97 sd); LiH (seed 1, 176 groups)
    -5.601911 against -5.592862, sd 0.034270 (-0.26 sd); random8 (seed 3, 26 groups) -2.280601 against -2.211519, sd 0.073400
    (-0.94 sd)."""
    shots = 4096
    c = mc.energy_case(name)
    xs, zs, cs, const = c.packed()
    norm1 = np.abs(cs).sum() + abs(const)
    with SV(c.n) as sv:
        c.load(sv)
        plan = sv.measurement_groups()
        mc.check_plan(c.n, xs, zs, cs, *plan)
        for got, want in zip(plan, mc.plan_groups(xs, zs, cs)):
            assert np.array_equal(got, want)
        G = len(plan[1])
        sv.prepare_state(c.theta)
        prepared = sv.get_state()
        e_dev, s_dev = sv.energy_sampled(c.theta, shots, seed=c.seed)
        info = sv.measure_info()
        psi = sv.get_state()
        assert np.array_equal(_bits(psi), _bits(prepared))                      # exactly what prepare_state leaves
        assert info["groups"] == G and info["shots"] == shots and info["terms"] == int(np.count_nonzero(plan[0] >= 0)), info
        assert (e_dev, s_dev) == sv.energy_sampled(c.theta, shots, seed=c.seed)  # bit-identical from call to call
        assert e_dev != sv.energy_sampled(c.theta, shots, seed=c.seed + 1)[0]
        e_rep, s_rep, outs, _, probs = mc.replay_energy(psi, c.n, xs, zs, cs, const, plan, shots, c.seed)
        # the device's own outcomes, group by group (stream = group, shots 0 .. n - 1): acceptance rule, eps-margin shots, and the
        # estimate re-assembled from the groups' sums
        margin, sum_v, sum_v2 = 0, [], []
        for g in range(G):
            members = mc.group_terms(plan[0], g)
            tm = [int(xs[t]) | int(zs[t]) for t in members]
            _, vsum, idx = sv.measure_paulis(tm, [cs[t] for t in members], shots, xbasis=int(plan[1][g]), ybasis=int(plan[2][g]), seed=c.seed,
                                             stream=g, return_indices=True)
            ok = np.array_equal(idx, outs[g])
            if not ok:
                margin += mc.check_outcomes(idx, probs[g], mc.uniforms(c.seed, g, 0, shots), f"{name} group {g}")
            sum_v.append(vsum[0]), sum_v2.append(vsum[1])
        e_sum, s_sum = mc.estimate(const + sum(cs[t] for t in range(len(xs)) if plan[0][t] < 0), shots, sum_v, sum_v2)
        bound = margin * 2 * np.abs(cs).sum() / shots + 1e-12 * norm1
        print(f"{name}: {G} groups, device {e_dev:.12f} +- {s_dev:.3e}, replay {e_rep:.12f} +- {s_rep:.3e}, {margin} margin shots, bound {bound:.3e}, info {info}")
        assert margin <= mc.MARGIN_SHARE * shots * G
        assert abs(e_dev - e_rep) <= bound and abs(s_dev - s_rep) <= bound
        assert abs(e_dev - e_sum) <= 1e-12 * norm1 and abs(s_dev - s_sum) <= 1e-12 * norm1
        e_exact, sd = mc.exact_moments(psi, c.n, xs, zs, cs, const, plan, shots)
        assert abs(e_exact - sv.energy(c.theta)) < 1e-10 * norm1
        assert abs(e_rep - e_exact) <= 3 * sd and abs(s_rep - sd) < 0.1 * sd


def test_zero_variance(SV):
    from openvqe_amd import fermion
    from openvqe_amd.operators import Hamiltonian, Term
    c = mc.energy_case("H2")
    zonly = Hamiltonian(4, [t for t in c.ham.terms if set(t.op) <= {"Z"}], c.ham.constant_coeff)
    with SV(4) as sv:                       # theta = 0: |hf>, an eigenstate of every Z string
        sv.set_hamiltonian(zonly)
        sv.set_ucc_program(fermion.uccsd_generators(2, 1), c.hf)
        e, s = sv.energy_sampled(np.zeros(3), 4096, seed=2)
        assert s == 0.0 and abs(e - sv.energy(np.zeros(3))) < 1e-14 and abs(e - (-1.0716472822963232)) < 1e-13
        assert sv.measure_info()["groups"] == 1
    n = 5
    with SV(n) as sv:                       # one X...X term on |+>^n
        sv.set_hamiltonian(Hamiltonian(n, [Term(-0.7, "X" * n, list(range(n)))], 0.25))
        sv.set_gate_program([("H", [q], 0.0, 0.0, -1) for q in range(n)], 0, 0)
        e, s = sv.energy_sampled(np.zeros(0), 1024, seed=5)
        assert s == 0.0 and abs(e - (-0.45)) < 1e-15
        group, xb, yb = sv.measurement_groups()
        assert list(group) == [0] and list(xb) == [(1 << n) - 1] and list(yb) == [0]


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals(SV):
    from openvqe_amd import fermion
    c = mc.energy_case("H2")
    with SV(4) as sv:
        sv.init_basis(3)
        for xb, yb in ((1, 1), (0b0110, 0b0100), (16, 0), (0, 1 << 63)):
            code, msg = _code(lambda: sv.measure_paulis([1], [1.0], 10, xbasis=xb, ybasis=yb))
            assert code == INVALID and "disjoint" in msg
        code, msg = _code(lambda: sv.measure_paulis([1], [1.0], -1))
        assert code == INVALID and "n_shots" in msg
        code, msg = _code(lambda: sv.energy_sampled([], 100))                 # neither Hamiltonian nor program
        assert code == STATE
        assert _code(lambda: sv.measurement_groups())[0] == STATE
        sv.set_hamiltonian(c.ham)
        code, msg = _code(lambda: sv.energy_sampled([], 100))
        assert code == STATE and "program" in msg
        sv.set_ucc_program(fermion.uccsd_generators(2, 1), c.hf)
        for shots in (0, 1):
            code, msg = _code(lambda: sv.energy_sampled(c.theta, shots))
            assert code == INVALID and "n_shots" in msg
        assert sv.energy_sampled(c.theta, 2)[1] >= 0.0
        sv.set_state(np.zeros(16))                                            # the zero state
        for call in (lambda: sv.sample(10), lambda: sv.sample(0), lambda: sv.measure_paulis([1], [1.0], 10, xbasis=1)):
            code, msg = _code(call)
            assert code == STATE and "weight" in msg
        sv.set_option("real_state", 1)
        for call in (lambda: sv.sample(10), lambda: sv.measure_paulis([1], [1.0], 10), lambda: sv.energy_sampled(c.theta, 10),
                     lambda: sv.measurement_groups()):
            code, msg = _code(call)
            assert code == STATE and "real_state" in msg
        sv.set_option("real_state", 0)
    with SV(4) as sv:                                                         # a program but no Hamiltonian
        sv.set_ucc_program(fermion.uccsd_generators(2, 1), c.hf)
        code, msg = _code(lambda: sv.energy_sampled(c.theta, 100))
        assert code == STATE and "Hamiltonian" in msg
        assert all(v == 0 for v in sv.measure_info().values())
    with SV(4, n_global=1, shard_index=0) as sv:
        for call in (lambda: sv.sample(10), lambda: sv.measure_paulis([1], [1.0], 10), lambda: sv.measurement_groups()):
            code, msg = _code(call)
            assert code == STATE and "shard" in msg


# ---- through the stand-ins -------------------------------------------------------------------------------------------------------------
def test_hipqpu_jobs_with_shots(gpu_lib):
    from openvqe_amd import qat_compat as qc
    c = mc.energy_case("H2")
    prog = qc.Program()
    reg = prog.qalloc(4)
    prog.apply(qc.build_ucc_ansatz(c.gens, c.hf)(list(c.theta)), reg)
    circ = prog.to_circ()
    qpu, twin = qc.HipQPU(seed=3), qc.HipQPU(seed=3)
    exact = qpu.submit(circ.to_job(job_type="OBS", observable=c.ham))
    assert exact.error is None and abs(exact.value - (-1.1004188945834952)) < 1e-12
    amps = {s.state.int: s.amplitude for s in qpu.submit(circ.to_job())}
    assert abs(sum(abs(a) ** 2 for a in amps.values()) - 1) < 1e-12
    job = circ.to_job(job_type="OBS", observable=c.ham, nbshots=4096)
    r1, r2 = qpu.submit(job), qpu.submit(job)
    for _ in range(2):
        twin.submit(circ.to_job())
    t1 = twin.submit(job)
    assert (r1.value, r1.error) == (t1.value, t1.error) and r1.value != r2.value
    assert 0 < r1.error < 0.01 and abs(r1.value - exact.value) < 5 * r1.error and abs(r2.value - exact.value) < 5 * r2.error
    res = qpu.submit(circ.to_job(nbshots=2000))
    states = [s.state.int for s in res]
    assert states == sorted(set(states)) and set(states) <= set(amps) and all(s.amplitude is None for s in res)
    assert abs(sum(s.probability for s in res) - 1) < 1e-12 and max(res, key=lambda s: s.probability).state.int == c.hf
    assert qpu.submit(circ.to_job(job_type="OBS", observable=c.ham)).value == exact.value      # nbshots = 0 is unchanged
