"""GPU tests of deflated energies and gradients (ovqe_deflation_push / _truncate / _count, ovqe_deflated_gradient_batch, ovqe_deflation_info:
k_sparse_vqd_batch in csrc/sv_sparse.hpp, csrc/sv_deflate.hpp, deflate_host.inc, abi_deflate.inc) and of variational quantum deflation on
top of them (openvqe_amd/excited.py: vqd).

Bounds (tests/deflation_cases.py): with W = ||H||_1 + sum_j beta_j ||phi_j||^2 and C of tests/gradbatch_cases.py, 1e-10 W max(1, C) against
the checker, 1e-12 W max(1, C) against another call on the same handle, 1e-12 ||phi_j|| for an overlap.  Every path-1 call is also held to
``gradbatch_cases.check_info`` through the info entries it shares with ovqe_gradient_batch_info.  The checker's vectors are read back
from the handle (``get_state`` of the buffer that was pushed): what is compared is the evaluation, not the preparation of phi_j."""
import ctypes

import numpy as np
import pytest

from openvqe_amd import chem, excited, fermion
from openvqe_amd.backend import compile_ucc_program
from tests import deflation_cases as dc
from tests import gradbatch_cases as gc
from tests import hessian_cases, metric_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def SV(gpu_lib):
    from openvqe_amd.backend import Statevector
    return Statevector


def _molecule(symbol):
    mol = chem.molecule(symbol)
    mol.rhf()
    ham = mol.jw_hamiltonian()
    n = ham.nbqbits
    gens = fermion.uccsd_generators(mol.nao, mol.n_elec // 2)
    rx, rz, rc, rp, K = compile_ucc_program(n, gens)
    hf = mol.hf_init()
    hf = int(hf) if np.isscalar(hf) else int(sum(1 << (n - 1 - q) for q, v in enumerate(hf) if v))
    case = gc.Case(n, hf, rx, rz, rc, rp, K, ham=ham)
    case.gens = gens
    return case


@pytest.fixture(scope="module")
def h4():
    return _molecule("H4")


@pytest.fixture(scope="module")
def lih():
    return _molecule("LiH")


class Held:
    """the vectors a handle holds, as the checker sees them"""

    def __init__(self):
        self.vectors, self.betas = [], []

    def push_state(self, sv, beta):
        """whatever the buffer holds"""
        before = sv.get_state()
        sv.deflation_push(beta)
        assert np.array_equal(sv.get_state().view(np.int64), before.view(np.int64))     # the buffer is only read
        self.vectors.append(before)
        self.betas.append(float(beta))

    def push_ansatz(self, sv, theta, beta):
        sv.prepare_state(theta)
        self.push_state(sv, beta)

    def push_vector(self, sv, vector, beta):
        sv.set_state(vector)
        self.push_state(sv, beta)


def _call(sv, thetas, held):
    """deflated_gradient_batch with the checks every result gets -> (costs, grads, energies, overlaps, info)"""
    thetas = np.ascontiguousarray(thetas, np.float64)
    c, g, e, o = sv.deflated_gradient_batch(thetas)
    info = sv.deflation_info()
    B, K = thetas.shape
    J = len(held.vectors)
    assert c.shape == e.shape == (B,) and g.shape == (B, K) and o.shape == (B, J) and o.dtype == np.complex128
    assert all(np.all(np.isfinite(a)) for a in (c, g, e, o.view(np.float64)))
    assert (info["B"], info["K"], info["J"]) == (B, K, J) and sv.deflation_count() == J, info
    pen = np.array([sum(b * abs(x) ** 2 for b, x in zip(held.betas, row)) for row in o]).reshape(B)
    assert np.abs(c - e - pen).max() <= 1e-13 * dc.weight(1.0, held.vectors, held.betas)     # cost = energy + penalty of the returned overlaps
    return c, g, e, o, info


def _against_checker(case, held, thetas, out, rows, want=None):
    c, g, e, o = out[:4]
    tol = dc.bound_checker(case.h1, case.C, held.vectors, held.betas)
    for b in rows:
        cw, gw, ew, ow = dc.case_want(case, thetas[b], held.vectors, held.betas) if want is None else want(thetas[b])
        dcost, de, dg = abs(c[b] - cw), abs(e[b] - ew), float(np.abs(g[b] - gw).max(initial=0.0))
        do = [abs(x - y) for x, y in zip(o[b], ow)]
        print(f"   row {b} against the checker: |dC| {dcost:.3e} |dE| {de:.3e} max|dg| {dg:.3e} bound {tol:.3e}; overlaps {[f'{x:.1e}' for x in do]}; "
              f"penalty {cw - ew:.4f} max|g| {np.abs(gw).max(initial=0.0):.4f}")
        assert dcost <= tol and de <= tol and dg <= tol
        for x, v in zip(do, held.vectors):
            assert x <= dc.bound_overlap(v)


def _against_single_rows(sv, case, held, thetas, out, rows):
    c, g, e, o = out[:4]
    tol = dc.bound_single(case.h1, case.C, held.vectors, held.betas)
    for b in rows:
        c1, g1, e1, o1 = sv.deflated_gradient_batch(thetas[b:b + 1])
        assert abs(c1[0] - c[b]) <= tol and abs(e1[0] - e[b]) <= tol and np.abs(g1[0] - g[b]).max(initial=0.0) <= tol
        assert all(abs(x - y) <= dc.bound_overlap(v) for x, y, v in zip(o1[0], o[b], held.vectors))


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def _sizes(sv, info, K):
    """(slots, ntab, nops, npairs, K) of the handle's compact program, the table entries from the LDS bytes of this launch"""
    pi = sv.program_info()
    m, nops, npairs = gc.slots(info["support"]), pi["sp_ops"], pi["sp_pairs"]
    stride, rest = divmod(info["lds_bytes"] - (nops * 16 + npairs * 4 if info["form"] == 1 else 0), info["waves"])
    assert rest == 0 and stride % 16 == 0 and pi["support"] == info["support"], info
    ntab = (stride - 2 * ((m + 1) & ~1) * 8 - ((K + 1) & ~1) * 8) // 24
    assert gc.wave_stride(m, ntab, K) == stride, (info, pi, ntab)
    return m, ntab, nops, npairs, K


def _path1(sv, info, K, B, waves=0, workgroups=0, sizes=None):
    sizes = _sizes(sv, info, K) if sizes is None else sizes
    gc.check_info(info, sizes, B, waves=waves, workgroups=workgroups)
    return sizes


# ---- path 1 ------------------------------------------------------------------------------------------------------------------------------
def test_no_vectors_is_the_batched_gradient(SV, h4):
    """H4, B = 7, nothing pushed: costs and energies are ovqe_energy_gradient_batch's to the bit, gradients within the same-handle bound,
    the overlaps array is not touched; and the same with one vector of weight 0"""
    thetas = np.random.default_rng(70).uniform(-0.3, 0.3, (7, h4.K))
    held = Held()
    with SV(h4.n) as sv:
        sv.set_hamiltonian(h4.ham)
        sv.set_ucc_program(h4.gens, h4.hf)
        e0, g0 = sv.energy_gradient_batch(thetas)
        for round_ in range(2):
            c, g, e, o, info = _call(sv, thetas, held)
            _path1(sv, info, h4.K, 7)
            assert info["rows"] == len(held.vectors) and _same_bits(c, e0) and _same_bits(e, e0)
            assert np.abs(g - g0).max() <= h4.tol_single()
            if round_ == 0:
                costs, grads, tail = np.zeros(7), np.zeros(7 * h4.K), np.full(16, -7.25)
                assert sv._L.ovqe_deflated_gradient_batch(sv._h, 7, thetas, h4.K, costs, grads, None, tail) == 0
                assert np.all(tail == -7.25) and _same_bits(costs, e0) and info["gather_launches"] == 0
                held.push_ansatz(sv, thetas[2], 0.0)
            else:
                assert abs(abs(o[2, 0]) - 1.0) <= 1e-12 and info["gather_launches"] == 1


@pytest.mark.parametrize("which", ["no_active_op", "two_states"])
def test_smallest_supports(SV, which):
    """m = 1 and m = 2 with psi(theta_0) pushed: at theta_0 the overlap is 1, the cost E + beta and the gradient the undeflated one (the
    overlap is stationary there); elsewhere the checker"""
    case, _ = getattr(gc, which)()
    thetas = np.random.default_rng(len(which)).uniform(-0.6, 0.6, (3, case.K))
    held, beta = Held(), 1.75
    with SV(case.n) as sv:
        case.load(sv)
        held.push_ansatz(sv, thetas[0], beta)
        out = _call(sv, thetas, held)
        c, g, e, o, info = out
        _path1(sv, info, case.K, 3)
        e0, g0 = sv.energy_gradient_batch(thetas[:1])
    print(f"{which}: {info}")
    assert info["support"] == (1 if which == "no_active_op" else 2) and info["rows"] == 1
    assert abs(o[0, 0] - 1.0) <= dc.bound_overlap(held.vectors[0])
    tol = dc.bound_single(case.h1, case.C, held.vectors, held.betas)
    assert abs(e[0] - e0[0]) <= tol and abs(c[0] - e0[0] - beta) <= tol and np.abs(g[0] - g0[0]).max(initial=0.0) <= tol
    _against_checker(case, held, thetas, out, range(3))


@pytest.fixture(scope="module")
def lih_rows(lih):
    return np.random.default_rng(12).uniform(-0.2, 0.2, (41, lih.K))


@pytest.mark.parametrize("nw", [1, 2, 4, 8])
def test_lih_every_wave_count(SV, lih, lih_rows, nw):
    """LiH UCCSD (m = 225 in 256 slots, K = 92) under "grad_batch_waves" = nw with J = 2 — an ansatz state and a random complex dense
    vector: three real rows, weight off the support — B = nw + 1, and B = 5 nw + 1 on two workgroups: idle waves, second and third
    trips.  Rows against the checker and against single-row calls; equal rows give equal bits"""
    held = Held()
    with SV(lih.n) as sv:
        sv.set_option("grad_batch_waves", nw)
        sv.set_hamiltonian(lih.ham)
        sv.set_ucc_program(lih.gens, lih.hf)
        held.push_ansatz(sv, lih_rows[40], 1.5)
        held.push_vector(sv, dc.random_vector(lih.n, 77), 2.5)
        sizes = None
        for B, wgs in ((nw + 1, 0), (5 * nw + 1, 2)):
            sv.set_option("grad_batch_workgroups", wgs)
            thetas = lih_rows[:B].copy()
            thetas[B - 1] = thetas[0]
            out = _call(sv, thetas, held)
            c, g, e, o, info = out
            sizes = _path1(sv, info, lih.K, B, waves=nw, workgroups=wgs, sizes=sizes)
            print(f"LiH nw = {nw} B = {B}: {info}")
            assert info["support"] == 225 and sizes[0] == 256 and info["waves"] == nw and info["rows"] == 3
            assert info["workgroups"] == (2 if wgs else -(-B // nw)) and info["gather_launches"] == (0 if wgs else 1)
            assert _same_bits(c[0], c[B - 1]) and _same_bits(e[0], e[B - 1]) and _same_bits(o[0].view(np.float64), o[B - 1].view(np.float64))
            _against_checker(lih, held, thetas, out, [0, 1] if wgs == 0 else [B - 2])
            _against_single_rows(sv, lih, held, thetas, out, [0, B // 2, B - 1])


@pytest.mark.parametrize("which", ["two_staged", "two_plain", "path2_first"])
def test_4096_states(SV, which):
    """m = 4096 on 12 qubits (every lane owns 64 slots), B = 3: J = 5 with one complex vector — six real rows — and J = 8 — nine, one
    past a group of eight — on the staged and the unstaged instance, and on the first program that falls to path 2"""
    R = gc.y_boundaries()[which]
    case, sizes = gc.y_program(R), gc.y_sizes(R)
    thetas = np.random.default_rng(R).uniform(-0.7, 0.7, (3, case.K))
    held = Held()
    with SV(case.n) as sv:
        case.load(sv)
        for j in range(8):
            held.push_vector(sv, dc.random_vector(case.n, 100 + j, real=j != 3), 0.5 + 0.25 * j)
            if j not in (4, 7) or (j == 7 and which == "path2_first"):
                continue
            out = _call(sv, thetas, held)
            info = out[4]
            print(f"{which} R = {R} J = {j + 1}: {info}")
            if which == "path2_first":
                assert info["path"] == 2 and not any(info[k] for k in ("rows", "form", "waves", "workgroups", "lds_bytes", "gather_launches"))
            else:
                _path1(sv, info, case.K, 3, sizes=sizes)
                assert info["rows"] == j + 2 and info["form"] == (1 if which == "two_staged" else 2) and info["gather_launches"] == 1
            _against_checker(case, held, thetas, out, [1])


def test_gather_cache(SV, h4):
    """the rows are gathered when the set of vectors or the compact program changed, and only then"""
    n, hf, gens, K = 8, h4.hf, h4.gens, h4.K
    thetas = np.random.default_rng(3).uniform(-0.3, 0.3, (2, K))
    held = Held()
    with SV(n) as sv:
        sv.set_hamiltonian(h4.ham)
        sv.set_ucc_program(gens, hf)
        held.push_vector(sv, dc.random_vector(n, 5), 1.25)
        assert _call(sv, thetas, held)[4]["gather_launches"] == 1
        assert _call(sv, thetas, held)[4]["gather_launches"] == 0
        other = gc.per_rotation(9)                          # 7 qubits of the 8: another support
        sv.set_rotation_program(other.rx, other.rz, other.rc, other.pidx, other.K, other.hf)
        case = gc.Case(n, other.hf, other.rx, other.rz, other.rc, other.pidx, other.K, ham=h4.ham)
        th = np.random.default_rng(4).uniform(-0.6, 0.6, (2, other.K))
        out = _call(sv, th, held)
        assert out[4]["path"] == 1 and out[4]["gather_launches"] == 1 and out[4]["support"] == 128
        _against_checker(case, held, th, out, [0, 1])
        assert _call(sv, th, held)[4]["gather_launches"] == 0
        held.push_ansatz(sv, th[1], 0.75)
        out = _call(sv, th, held)
        assert out[4]["gather_launches"] == 1 and out[4]["rows"] == 3
        _against_checker(case, held, th, out, [0])
        sv.deflation_truncate(1)
        del held.vectors[1:], held.betas[1:]
        assert _call(sv, th, held)[4]["gather_launches"] == 1


# ---- path 2 ------------------------------------------------------------------------------------------------------------------------------
def _path2(info, J):
    assert info["path"] == 2 and info["J"] == J and info["launches"] == info["B"] * (2 * -(-J // 4) + J), info
    assert not any(info[k] for k in ("rows", "form", "waves", "workgroups", "lds_bytes", "support", "gather_launches")), info


def test_path_2_forced_on_h4_five_vectors(SV, h4):
    """J = 5 crosses the four-per-pass chunk of k_deflate_dots / k_deflate_axpy; the call is bit-identical from call to call"""
    thetas = np.random.default_rng(9).uniform(-0.3, 0.3, (3, h4.K))
    held = Held()
    with SV(h4.n) as sv:
        sv.set_option("force_path", 2)
        sv.set_hamiltonian(h4.ham)
        sv.set_ucc_program(h4.gens, h4.hf)
        held.push_ansatz(sv, thetas[1], 2.0)
        for j in range(4):
            held.push_vector(sv, dc.random_vector(h4.n, 20 + j, real=j == 2), 0.5 + j)
        out = _call(sv, thetas, held)
        _path2(out[4], 5)
        again = _call(sv, thetas, held)
        _against_single_rows(sv, h4, held, thetas, out, [0, 2])
    assert all(_same_bits(a.view(np.float64), b.view(np.float64)) for a, b in zip(out[:4], again[:4]))
    assert abs(out[3][1, 0] - 1.0) <= dc.bound_overlap(held.vectors[0])
    _against_checker(h4, held, thetas, out, range(3))


def test_path_2_tied_program(SV):
    """a complex program with a constant rotation, an offset, a tied and an unused parameter: the unused column is exact zeros"""
    n, hf, rx, rz, rc, pidx, phi0, K = metric_cases.tied_program()
    case = gc.Case(n, hf, rx, rz, rc, pidx, K, phi0=phi0, nterms=24, seed=17)
    thetas = np.random.default_rng(5).uniform(-0.8, 0.8, (3, K))
    held = Held()
    with SV(n) as sv:
        case.load(sv)
        held.push_ansatz(sv, thetas[2], 1.5)
        held.push_vector(sv, dc.random_vector(n, 6), 2.0)
        out = _call(sv, thetas, held)
        _path2(out[4], 2)
    _against_checker(case, held, thetas, out, range(3))
    assert not out[1][:, 4].any() and np.abs(out[1][:, 0]).min() > 1e-4


def test_path_2_literal_gate_list(SV):
    n, hf, gates, K = metric_cases.gate_list(False)
    hx, hz, hc = hessian_cases.random_real_hamiltonian(n, 16, 23)
    ham = hessian_cases.hamiltonian_object(n, hx, hz, hc, 0.1)

    class G:
        h1 = hessian_cases.norm1(hc, 0.1)
        C = max(sum(0.5 * abs(g[2]) for g in gates if g[4] == k) for k in range(K))

    thetas = np.random.default_rng(6).uniform(-0.8, 0.8, (3, K))
    held = Held()
    with SV(n) as sv:
        sv.set_option("clifford_frame", 0)
        sv.set_hamiltonian(ham)
        sv.set_gate_program(gates, K, hf)
        assert sv.program_info()["literal_gates"] > 0
        held.push_ansatz(sv, thetas[0], 1.25)
        held.push_vector(sv, dc.random_vector(n, 9), 0.5)
        out = _call(sv, thetas, held)
        _path2(out[4], 2)
    assert abs(out[3][0, 0] - 1.0) <= dc.bound_overlap(held.vectors[0])
    _against_checker(G, held, thetas, out, range(3),
                     want=lambda t: dc.deflated_gradient_gates(n, hf, gates, t, hx, hz, hc, 0.1, held.vectors, held.betas))


def test_path_2_beside_the_sector_tables(SV):
    """a program whose single gradient runs on the sector tables: the deflated call streams, meets the checker, and the single call
    still reports its sector forms afterwards"""
    from tests import sector_cases as sc
    case = sc.molecule(7, 2)
    theta = np.array(case.thetas(2)[:1])
    held = Held()
    with SV(case.n) as sv:
        for k, v in {"force_path": 2, "sector_min_qubits": 8}.items():
            sv.set_option(k, v)
        sv.set_hamiltonian(case.ham)
        sv.set_ucc_program(case.gens, case.hf)
        es, gs = sv.energy_gradient(theta[0])
        forms = sv.sector_forms()
        assert forms
        held.push_vector(sv, dc.random_vector(case.n, 14), 3.0)
        out = _call(sv, theta, held)
        _path2(out[4], 1)
        es2, gs2 = sv.energy_gradient(theta[0])
        assert sv.sector_forms() == forms and abs(es - es2) <= 1e-12 * case.bound and np.abs(gs - gs2).max() <= 1e-12 * case.bound
    assert abs(out[2][0] - es) <= 1e-10 * case.bound
    cw, gw, ew, ow = dc.deflated_gradient(case.n, case.hf, case.rx, case.rz, case.rc, case.pidx, theta[0], case.hx, case.hz, case.hc,
                                          float(np.real(case.ham.constant_coeff or 0.0)), None, held.vectors, held.betas)
    const = float(np.real(case.ham.constant_coeff or 0.0))
    tol = dc.bound_checker(hessian_cases.norm1(case.hc, const), hessian_cases.coefficient_sum(case.rc, case.pidx, case.K), held.vectors, held.betas)
    print(f"sector case: |dC| {abs(out[0][0] - cw):.3e} max|dg| {np.abs(out[1][0] - gw).max():.3e} bound {tol:.3e}")
    assert abs(out[0][0] - cw) <= tol and abs(out[2][0] - ew) <= tol and np.abs(out[1][0] - gw).max() <= tol
    assert abs(out[3][0, 0] - ow[0]) <= dc.bound_overlap(held.vectors[0])


# ---- contract ----------------------------------------------------------------------------------------------------------------------------
SENTINEL = -7.25
INVALID, STATE = -1, -5


def _raw(sv, B, theta, K, costs, grads, energies, overlaps):
    rc = sv._L.ovqe_deflated_gradient_batch(sv._h, B, theta, K, costs, grads, energies, overlaps)
    return rc, (sv._L.ovqe_last_error(sv._h) or b"").decode()


@pytest.mark.parametrize("path", [1, 2])
def test_bounds_of_the_five_arrays(SV, h4, path):
    """theta with a NaN tail, the four outputs with sentinel tails: finite results, untouched sentinels"""
    B, K, J = 5, h4.K, 2
    rows = np.random.default_rng(15).uniform(-0.3, 0.3, (B, K))
    theta = np.concatenate([rows.reshape(-1), np.full(3 * K, np.nan)])
    costs, energies, grads, overlaps = np.full(B + 16, SENTINEL), np.full(B + 16, SENTINEL), np.full(B * K + 64, SENTINEL), np.full(2 * B * J + 32, SENTINEL)
    held = Held()
    with SV(h4.n) as sv:
        sv.set_option("force_path", 2 if path == 2 else 0)
        sv.set_hamiltonian(h4.ham)
        sv.set_ucc_program(h4.gens, h4.hf)
        held.push_ansatz(sv, rows[0], 1.0)
        held.push_vector(sv, dc.random_vector(h4.n, 2), 2.0)
        rc, msg = _raw(sv, B, theta, K, costs, grads, energies, overlaps)
        assert rc == 0, msg
        assert sv.deflation_info()["path"] == path
        c, g, e, o = sv.deflated_gradient_batch(rows)
    for arr, used in ((costs, B), (energies, B), (grads, B * K), (overlaps, 2 * B * J)):
        assert np.all(np.isfinite(arr[:used])) and np.all(arr[used:] == SENTINEL)
    tol = dc.bound_single(h4.h1, h4.C, held.vectors, held.betas)
    assert np.abs(costs[:B] - c).max() <= tol and np.abs(grads[:B * K] - g.reshape(-1)).max() <= tol
    assert np.abs(overlaps[:2 * B * J] - o.view(np.float64).reshape(-1)).max() <= 1e-12


def test_refusals_and_the_empty_batch(SV):
    n, hf, rx, rz, rc, pidx, phi0, K = metric_cases.tied_program()
    case = gc.Case(n, hf, rx, rz, rc, pidx, K, phi0=phi0, nterms=24, seed=17)
    theta, c, e, g, o = np.zeros(2 * K), np.full(2, SENTINEL), np.full(2, SENTINEL), np.full(2 * K, SENTINEL), np.full(8, SENTINEL)

    def refused(sv, code, text, *args):
        rc, msg = _raw(sv, *args)
        assert rc == code and text in msg, (rc, msg)

    def last(sv):
        return (sv._L.ovqe_last_error(sv._h) or b"").decode()

    with SV(n) as sv:
        info = (ctypes.c_int64 * 14)(*([7] * 14))
        assert sv._L.ovqe_deflation_info(sv._h, info, 14) == 0 and not any(info)          # zeros before the first call
        refused(sv, STATE, "no program set", 2, theta, K, c, g, e, o)
        sv.set_rotation_program(rx, rz, rc, pidx, K, hf, phi0=phi0)
        refused(sv, STATE, "no Hamiltonian set", 2, theta, K, c, g, e, o)
        sv.set_hamiltonian(case.ham)
        refused(sv, INVALID, "K does not match", 2, theta, K - 1, c, g, e, o)
        refused(sv, INVALID, "B is negative", -1, theta, K, c, g, e, o)
        refused(sv, INVALID, "theta is NULL", 2, None, K, c, g, e, o)
        refused(sv, INVALID, "costs is NULL", 2, theta, K, None, g, e, o)
        refused(sv, INVALID, "grads is NULL", 2, theta, K, c, None, e, o)
        sv.set_option("real_state", 1)
        refused(sv, STATE, "real_state", 2, theta, K, c, g, e, o)
        assert sv._L.ovqe_deflation_push(sv._h, 1.0) == STATE and "real_state" in last(sv)
        sv.set_option("real_state", 0)
        # the vectors: weights, the 33rd, truncation at its edges
        for bad in (-0.5, np.nan, np.inf):
            assert sv._L.ovqe_deflation_push(sv._h, bad) == INVALID and "beta" in last(sv)
        count = ctypes.c_int32(-1)
        assert sv._L.ovqe_deflation_count(sv._h, ctypes.byref(count)) == 0 and count.value == 0
        assert sv._L.ovqe_deflation_truncate(sv._h, 0) == 0 and sv._L.ovqe_deflation_truncate(sv._h, 1) == INVALID and "outside 0 .. 0" in last(sv)
        assert sv._L.ovqe_deflation_truncate(sv._h, -1) == INVALID
        sv.init_basis(hf)
        for j in range(32):
            assert sv.deflation_push(0.5) == j + 1
        assert sv._L.ovqe_deflation_push(sv._h, 0.5) == INVALID and "at most 32" in last(sv) and sv.deflation_count() == 32
        assert sv._L.ovqe_deflation_truncate(sv._h, 33) == INVALID and "outside 0 .. 32" in last(sv)
        sv.deflation_truncate(32)
        assert sv.deflation_count() == 32
        sv.deflation_truncate(3)
        assert sv.deflation_count() == 3
        sv.deflation_truncate()
        assert sv.deflation_count() == 0
        assert sv._L.ovqe_deflation_info(sv._h, info, 14) == 0 and not any(info)          # refused calls leave no figures
        # B = 0: OVQE_OK, nothing touched, NULL arrays allowed
        assert _raw(sv, 0, None, K, None, None, None, None)[0] == 0 and _raw(sv, 0, theta, K, c, g, e, o)[0] == 0
        assert all(np.all(a == SENTINEL) for a in (c, g, e, o))
        assert sv._L.ovqe_deflation_info(sv._h, info, 14) == 0 and not any(info)
        out = sv.deflated_gradient_batch(np.zeros((0, K)))
        assert [a.shape for a in out] == [(0,), (0, K), (0,), (0, 0)]
        # energies and overlaps may be NULL
        sv.deflation_push(1.0)
        assert _raw(sv, 2, theta, K, c, g, None, None)[0] == 0 and np.all(c != SENTINEL) and np.all(e == SENTINEL) and np.all(o == SENTINEL)
        assert sv._L.ovqe_deflation_info(sv._h, info, 14) == 0 and list(info)[:5] == [2, 2, K, 1, 0]
        assert sv._L.ovqe_deflation_info(sv._h, info, -1) == INVALID and sv._L.ovqe_deflation_info(sv._h, None, 14) == INVALID
        for bad in (np.zeros(K), np.zeros((2, K + 1)), np.zeros((1, 2, K))):
            with pytest.raises(ValueError):
                sv.deflated_gradient_batch(bad)
    with SV(n - 1, n_global=1, shard_index=0) as shard:
        assert shard._L.ovqe_deflation_push(shard._h, 1.0) == STATE and "shard" in last(shard)
        rc, msg = _raw(shard, 2, theta, K, c, g, e, o)
        assert rc != 0 and rc == shard._L.ovqe_energy_gradient_batch(shard._h, 2, theta, K, e, g), (rc, msg)


def test_open_clifford_frame_is_refused(SV):
    n, hf, gates, K = metric_cases.gate_list(True)
    hx, hz, hc = hessian_cases.random_real_hamiltonian(n, 16, 23)
    theta, c, g = np.zeros(K), np.zeros(1), np.zeros(K)
    with SV(n) as sv:
        sv.set_hamiltonian(hessian_cases.hamiltonian_object(n, hx, hz, hc, 0.1))
        sv.set_gate_program(gates, K, hf)
        rc, msg = _raw(sv, 1, theta, K, c, g, None, None)
        assert rc == STATE and "clifford_frame" in msg and "open" in msg, (rc, msg)
        sv.set_option("clifford_frame", 0)
        sv.set_gate_program(gates, K, hf)
        rc, msg = _raw(sv, 1, theta, K, c, g, None, None)
        assert rc == 0, msg
    want = dc.deflated_gradient_gates(n, hf, gates, theta, hx, hz, hc, 0.1)
    assert abs(c[0] - want[0]) <= 1e-10 * hessian_cases.norm1(hc, 0.1)


def test_vectors_survive_a_new_hamiltonian_and_program(SV, h4):
    thetas = np.random.default_rng(21).uniform(-0.3, 0.3, (2, h4.K))
    held = Held()
    with SV(h4.n) as sv:
        sv.set_hamiltonian(h4.ham)
        sv.set_ucc_program(h4.gens, h4.hf)
        held.push_ansatz(sv, thetas[0], 1.5)
        held.push_vector(sv, dc.random_vector(h4.n, 8), 0.5)
        first = _call(sv, thetas, held)
        sv.set_hamiltonian(h4.ham)
        sv.set_ucc_program(h4.gens, h4.hf)
        assert sv.deflation_count() == 2
        out = _call(sv, thetas, held)
    assert _same_bits(first[0], out[0]) and _same_bits(first[3].view(np.float64), out[3].view(np.float64))
    _against_checker(h4, held, thetas, out, [1])


@pytest.mark.parametrize("path", [0, 2])
def test_neighbours_untouched(SV, h4, path):
    """cached tables stay valid: energy and energy_batch before and after a deflated call to the bit, energy_gradient within 1e-13,
    the compact forms the handle reports unchanged"""
    theta = np.random.default_rng(9).uniform(-0.3, 0.3, h4.K)
    thetas = np.random.default_rng(10).uniform(-0.3, 0.3, (7, h4.K))
    with SV(h4.n) as sv:
        sv.set_option("force_path", path)
        sv.set_hamiltonian(h4.ham)
        sv.set_ucc_program(h4.gens, h4.hf)
        e0 = sv.energy(theta)
        b0 = sv.energy_batch(np.tile(theta, (3, 1)))
        ge0 = sv.energy_gradient(theta)
        forms, geometries = sv.sparse_forms(), sv.sparse_geometries()
        sv.prepare_state(theta)
        sv.deflation_push(2.0)
        sv.deflated_gradient_batch(thetas)
        assert sv.deflation_info()["path"] == (2 if path == 2 else 1)
        if path == 0:
            assert (sv.sparse_forms(), sv.sparse_geometries()) == (forms, geometries)
        e1 = sv.energy(theta)
        b1 = sv.energy_batch(np.tile(theta, (3, 1)))
        ge1 = sv.energy_gradient(theta)
    assert np.float64(e0).view(np.int64) == np.float64(e1).view(np.int64)
    assert np.array_equal(b0.view(np.int64), b1.view(np.int64))
    assert abs(ge0[0] - ge1[0]) <= 1e-13 * h4.h1 and np.abs(ge0[1] - ge1[1]).max() <= 1e-13 * h4.h1


# ---- VQD ---------------------------------------------------------------------------------------------------------------------------------
def test_vqd_three_levels_on_the_device(SV):
    from tests.test_deflation_cases import check_three_levels
    with SV(3) as sv:
        dc.load_three_bits(sv)
        states = excited.vqd(sv, 3)
        print(sv.deflation_info())
        check_three_levels(states, sv)


def test_vqd_on_lih_above_the_lanczos_ground_state(SV, lih):
    """LiH, two states above the sector's Lanczos ground state as a given vector: path 1, accepted costs never rise, every returned theta
    is stationary to the tolerance in a single-row call, the returned overlaps are a fresh evaluation's, the set is what it was.

    One start, theta = 0: the run from the Hartree-Fock determinant keeps the reference's symmetry and reaches the tolerance in a few
    hundred iterations.  With eight starts the perturbed ones break that symmetry and reach lower costs (E about -7.7565 and -7.7405
    against the FCI ground state's -7.8810) along nearly flat directions: measured at tol 1e-6, spread 0.1, L-BFGS memories of 10, 30
    and 92 pairs and beta = 0.5, 1, 2 and the default 2 ||H||_1 = 24.7, the lowest-cost start still had max |gradient| between 2e-6 (5000
    iterations, 4.8 s) and 1e-4 (2000 iterations) when the iterations ran out, while theta = 0 always converged."""
    tol = 1e-6
    with SV(lih.n) as sv:
        sv.set_hamiltonian(lih.ham)
        sv.init_basis(lih.hf)
        e_fci = sv.sector_ground_state(tol=1e-12)[0]        # no program yet: the sector of |hf>; the vector survives set_ucc_program
        beta = 2.0 * sv.hamiltonian_norm1()
        held = Held()
        held.push_state(sv, beta)
        sv.set_ucc_program(lih.gens, lih.hf)
        states = excited.vqd(sv, 2, starts=1, tol=tol)
        assert sv.deflation_info()["path"] == 1 and sv.deflation_count() == 1
        print(f"LiH: FCI {e_fci:.10f}; VQD energies {[s['energy'] for s in states]} costs {[s['cost'] for s in states]} iterations "
              f"{[s['result'].nit for s in states]} calls {[s['result'].ncalls for s in states]}; {sv.deflation_info()}")
        for k, s in enumerate(states):
            assert s["result"].success and np.all(np.diff(s["result"].energies) <= 0.0) and s["overlaps"].shape == (1 + k,)
            c, g, e, o, _ = _call(sv, s["theta"][None, :], held)
            assert np.abs(g).max() <= tol
            bound = dc.bound_single(lih.h1, lih.C, held.vectors, held.betas)
            assert abs(c[0] - s["cost"]) <= bound and abs(e[0] - s["energy"]) <= bound
            assert all(abs(x - y) <= dc.bound_overlap(v) for x, y, v in zip(o[0], s["overlaps"], held.vectors))
            assert s["energy"] >= e_fci - 1e-9
            held.push_ansatz(sv, s["theta"], beta)       # what vqd held while it looked for the next state
        sv.deflation_truncate(1)
