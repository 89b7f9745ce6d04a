"""GPU tests of the exact energy Hessian (ovqe_energy_hessian: csrc/sv_hessian_host.hpp, k_sparse_hessian in csrc/sv_sparse.hpp,
csrc/sv_hessian.hpp, hessian_host.inc; Statevector.energy_hessian / hessian_info) against the checkers of tests/hessian_cases.py, and of
Newton trust-region VQE (openvqe_amd/common_files/newton.py, EnergyUCC.newton).

Tolerance against the checker: |delta H_bk| <= 1e-10 ||H||_1 max(1, C^2), C = max_k sum_{r in k} |coeff_r| — the project's 1e-10 ||H||_1
energy bound carried through two derivatives.  Every result is also symmetric to the bit, reports an asymmetry of its raw rows within
the same bound, and returns E and the gradient of ``energy_gradient`` within 1e-12 ||H||_1 (``hessian_cases.call_hessian``)."""
import ctypes

import numpy as np
import pytest
import scipy.optimize

from openvqe_amd import chem, fermion
from openvqe_amd.backend import compile_ucc_program
from openvqe_amd.operators import pack_terms
from tests import hessian_cases, metric_cases

pytestmark = pytest.mark.gpu

_call, _compare = hessian_cases.call_hessian, hessian_cases.compare


@pytest.fixture(scope="module")
def SV(gpu_lib):
    from openvqe_amd.backend import Statevector
    return Statevector


def _hf_index(n, hf):
    return int(hf) if np.isscalar(hf) else int(sum(1 << (n - 1 - q) for q, v in enumerate(hf) if v))


class Mol:
    def __init__(self, symbol):
        mol = chem.molecule(symbol)
        mol.rhf()
        self.ham = mol.jw_hamiltonian()
        self.n = self.ham.nbqbits
        self.hf = _hf_index(self.n, mol.hf_init())
        self.gens = fermion.uccsd_generators(mol.nao, mol.n_elec // 2)
        self.rx, self.rz, self.rc, self.rp, self.K = compile_ucc_program(self.n, self.gens)
        hx, hz, hc = pack_terms(self.n, self.ham.terms)
        self.h = (hx, hz, np.real(hc), float(np.real(self.ham.constant_coeff or 0.0)))
        self.h1 = hessian_cases.norm1(self.h[2], self.h[3])
        self.C = hessian_cases.coefficient_sum(self.rc, self.rp, self.K)

    def want(self, theta):
        return hessian_cases.hessian(self.n, self.hf, self.rx, self.rz, self.rc, self.rp, theta, *self.h)[2]


@pytest.fixture(scope="module")
def h4():
    return Mol("H4")


@pytest.fixture(scope="module")
def lih():
    return Mol("LiH")


class Synthetic:
    """a rotation program with a random real Hamiltonian (identity, Z-only and even-Y terms) whose x masks connect the program's support"""

    def __init__(self, n, hf, rx, rz, rc, pidx, phi0, K, nterms, seed):
        self.n, self.hf, self.K, self.phi0 = n, hf, K, phi0
        self.prog = (n, hf, rx, rz, rc, pidx)
        hx, hz, hc = hessian_cases.random_real_hamiltonian(n, nterms, seed, x_pool=rx)
        self.h = (hx, hz, hc, 0.25)
        self.ham = hessian_cases.hamiltonian_object(n, hx, hz, hc, 0.25)
        self.h1 = hessian_cases.norm1(hc, 0.25)
        self.C = hessian_cases.coefficient_sum(rc, pidx, K)

    def load(self, sv):
        n, hf, rx, rz, rc, pidx = self.prog
        sv.set_hamiltonian(self.ham)
        sv.set_rotation_program(rx, rz, rc, pidx, self.K, hf, phi0=self.phi0)

    def want(self, theta):
        return hessian_cases.hessian(*self.prog, theta, *self.h, self.phi0)[2]


# ---- compact support ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def h4_compact(SV, h4):
    """H4/STO-3G UCCSD, 8 qubits, at random theta and at theta = 0: the compact results the streaming test compares with"""
    theta = np.random.default_rng(8).uniform(-0.3, 0.3, h4.K)
    with SV(h4.n) as sv:
        sv.set_hamiltonian(h4.ham)
        sv.set_ucc_program(h4.gens, h4.hf)
        _, _, hs, info = _call(sv, theta, 1, h4.h1, h4.C)
        _, _, hs0, _ = _call(sv, np.zeros(h4.K), 1, h4.h1, h4.C)
    return theta, hs, hs0, info


def test_h4_uccsd_on_the_compact_support(h4, h4_compact):
    theta, hs, hs0, info = h4_compact
    _compare(hs, h4.want(theta), "H4 random theta", h4.h1, h4.C)
    _compare(hs0, h4.want(np.zeros(h4.K)), "H4 theta = 0", h4.h1, h4.C)
    assert info["launches"] == 1 and 0 < info["amplitudes"] <= 70 and info["form"] == 1 and info["entries"] > 0
    assert info["phase2_us"] == 0 and info["workspace_bytes"] == (h4.K * h4.K + h4.K + 1) * 8 + info["entries"] * 16


def test_lih_uccsd_92_directions(SV, lih):
    """12 qubits, 92 parameters, m = 225 (odd: mpad = 226): more than 64 workgroups in the one launch"""
    assert lih.n == 12 and lih.K == 92
    theta = np.random.default_rng(12).uniform(-0.2, 0.2, lih.K)
    with SV(lih.n) as sv:
        sv.set_hamiltonian(lih.ham)
        sv.set_ucc_program(lih.gens, lih.hf)
        _, _, hs, info = _call(sv, theta, 1, lih.h1, lih.C)
    _compare(hs, lih.want(theta), "LiH", lih.h1, lih.C)
    assert info["amplitudes"] == 225 and info["launches"] == 1 and info["K"] >= 64


@pytest.fixture(scope="module")
def synth_strings():
    _, gens, hf = fermion.synthetic_molecule(6, 3, 41)
    return gens, hf


@pytest.mark.parametrize("K", [1, 2, 65])
def test_block_and_grid_edges(SV, synth_strings, K):
    """one parameter per rotation, truncated to K, 12 qubits, a 20-term random real Hamiltonian: a lone workgroup, two, one more than a
    wave has lanes.  Direction K - 1 starts at the last op (the tangent is dropped below it), direction 0 at op 0"""
    gens, hf = synth_strings
    n = 12
    rx, rz, rc, rp = metric_cases.one_parameter_per_rotation(gens, n, K)
    case = Synthetic(n, hf, rx, rz, rc, rp, None, K, 20, 300 + K)
    theta = np.random.default_rng(K).uniform(-0.4, 0.4, K)
    with SV(n) as sv:
        case.load(sv)
        _, _, hs, info = _call(sv, theta, 1, case.h1, case.C)
    want = case.want(theta)
    _compare(hs, want, f"K = {K}", case.h1, case.C)
    _compare(hs[K - 1], want[K - 1], f"K = {K}: the direction whose first op is the last op", case.h1, case.C)
    _compare(hs[0], want[0], f"K = {K}: the direction whose first op is op 0", case.h1, case.C)
    assert info["launches"] == 1 and np.abs(want[K - 1]).max() > 1e-6


@pytest.fixture(scope="module")
def tied():
    n, hf, rx, rz, rc, pidx, phi0, K = metric_cases.tied_program()
    return Synthetic(n, hf, rx, rz, rc, pidx, phi0, K, 24, 17)


@pytest.fixture(scope="module")
def tied_compact(SV, tied):
    theta = np.random.default_rng(5).uniform(-0.8, 0.8, tied.K)
    with SV(tied.n) as sv:
        tied.load(sv)
        _, _, hs, _ = _call(sv, theta, 1, tied.h1, tied.C)
    return theta, hs


def test_tied_parameter_constant_rotation_and_unused_parameter(tied, tied_compact):
    """parameter 0 tied across non-adjacent rotations, a constant rotation between parameterised ones, an offset, an unused parameter
    (an exact zero row and column); the Hamiltonian holds an identity term, a Z-only term and even-Y terms"""
    theta, hs = tied_compact
    hx, hz, _, _ = tied.h
    assert (int(hx[0]), int(hz[0])) == (0, 0) and int(hx[1]) == 0 and any(bin(int(x) & int(z)).count("1") == 2 for x, z in zip(hx, hz))
    _compare(hs, tied.want(theta), "tied program", tied.h1, tied.C)
    assert not hs[4].any() and not hs[:, 4].any() and abs(hs[0, 0]) > 0.01


# ---- LDS boundaries at m = 4096 -----------------------------------------------------------------------------------------------------
CUBE_K = 6
CUBE_R = hessian_cases.cube_boundaries(12, CUBE_K)   # last staged, first unstaged, last unstaged, first streaming


@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_kernel_forms_at_the_support_cap(SV, which):
    """cube_program(12, R, 6, seed) with a 12-term Hamiltonian: four vectors of 4096 doubles take 128 KiB of the 150 KiB budget — the
    last program whose ops and pair words are staged, the first that reads them from global memory, the last that fits at all and the
    first that streams.  Form and LDS bytes against the formula"""
    R = CUBE_R[which]
    n, hf, rx, rz, rc, pidx, phi0, K = metric_cases.cube_program(12, R, CUBE_K, 100 + R)
    case = Synthetic(n, hf, rx, rz, rc, pidx, phi0, K, 12, 400 + which)
    form, lds = hessian_cases.hessian_form(*hessian_cases._cube(12, R, K))
    assert form == (1, 2, 2, 0)[which]
    theta = np.random.default_rng(R).uniform(-0.8, 0.8, K)
    with SV(n) as sv:
        case.load(sv)
        _, _, hs, info = _call(sv, theta, 1 if form else 2, case.h1, case.C)
    assert info["form"] == form and info["lds_bytes"] == lds and info["amplitudes"] == 4096, info
    _compare(hs, case.want(theta), f"cube_program(12, {R}) form {form}", case.h1, case.C)


# ---- streaming ----------------------------------------------------------------------------------------------------------------------
def test_streaming_agrees_with_the_compact_path(SV, h4, h4_compact, tied, tied_compact):
    theta, hs_compact, _, _ = h4_compact
    with SV(h4.n) as sv:
        sv.set_option("force_path", 2)
        sv.set_hamiltonian(h4.ham)
        sv.set_ucc_program(h4.gens, h4.hf)
        _, _, hs, info = _call(sv, theta, 2, h4.h1, h4.C)
        again = sv.energy_hessian(theta)[2]
    _compare(hs, hs_compact, "H4 streaming against compact", h4.h1, h4.C)
    assert np.array_equal(hs.view(np.int64), again.view(np.int64))   # fixed-order sums: the same bits from call to call
    assert info["amplitudes"] == 256 and info["form"] == 0 and info["lds_bytes"] == 0 and info["phase2_us"] > 0
    assert info["workspace_bytes"] == hessian_cases.streaming_workspace(8, h4.K, len(h4.rx) + 1) == 2 * 256 * 64 * 16 + 64 * 64 * 8 + 161 * 64 * 8
    theta, hs_compact = tied_compact
    with SV(tied.n) as sv:
        sv.set_option("force_path", 2)
        tied.load(sv)
        _, _, hs, _ = _call(sv, theta, 2, tied.h1, tied.C)
    _compare(hs, hs_compact, "tied program streaming against compact", tied.h1, tied.C)
    assert not hs[4].any() and not hs[:, 4].any()


def test_gate_list_literal_and_frame_form(SV):
    """5 qubits, RY / RZ / CNOT with ascale = -2 on a shared parameter, an aconst offset and a leading RZ on a qubit still in |0>:
    the literal list and the Clifford-frame form against the gate checker"""
    n, hf, gates, K = metric_cases.gate_list(False)
    hx, hz, hc = hessian_cases.random_real_hamiltonian(n, 16, 23)
    ham = hessian_cases.hamiltonian_object(n, hx, hz, hc, 0.1)
    h1 = hessian_cases.norm1(hc, 0.1)
    C = max(sum(0.5 * abs(g[2]) for g in gates if g[4] == k) for k in range(K))
    theta = np.random.default_rng(6).uniform(-0.8, 0.8, K)
    want = hessian_cases.gate_hessian(n, hf, gates, theta, hx, hz, hc, 0.1)[2]
    assert np.abs(want[0]).max() < 1e-14 * h1 and abs(want[1, 1]) > 1e-3
    for frame in (1, 0):
        with SV(n) as sv:
            sv.set_option("clifford_frame", frame)
            sv.set_hamiltonian(ham)
            sv.set_gate_program(gates, K, hf)
            literal = sv.program_info()["literal_gates"]
            _, _, hs, _ = _call(sv, theta, 2, h1, C)
        assert (literal > 0) == (frame == 0), (frame, literal)
        _compare(hs, want, f"gate list clifford_frame = {frame}", h1, C)


# ---- contract -----------------------------------------------------------------------------------------------------------------------
def _refused(sv, rc_want, text, theta, K, hess, energy=True):
    e = ctypes.c_double()
    rc = sv._L.ovqe_energy_hessian(sv._h, theta, K, ctypes.byref(e) if energy else None, None, hess, None)
    msg = (sv._L.ovqe_last_error(sv._h) or b"").decode()
    assert rc == rc_want and text in msg, (rc, msg)


def test_refusals(SV, tied):
    INVALID, STATE = -1, -5
    n, hf, rx, rz, rc, pidx = tied.prog
    K = tied.K
    theta, out = np.zeros(K), np.zeros(K * K)
    with SV(n) as sv:
        info = (ctypes.c_int64 * 11)(*([7] * 11))
        assert sv._L.ovqe_hessian_info(sv._h, info, 11) == 0 and not any(info)            # zeros before the first call
        _refused(sv, STATE, "no program set", theta, K, out)
        sv.set_rotation_program(rx, rz, rc, pidx, K, hf, phi0=tied.phi0)
        _refused(sv, STATE, "no Hamiltonian set", theta, K, out)
        sv.set_hamiltonian(tied.ham)
        _refused(sv, INVALID, "K = 4", theta, K - 1, out)
        _refused(sv, INVALID, "theta is NULL", None, K, out)
        _refused(sv, INVALID, "hess is NULL", theta, K, None)
        sv.set_option("real_state", 1)
        _refused(sv, STATE, "real_state", theta, K, out)
        sv.set_option("real_state", 0)
        assert sv._L.ovqe_energy_hessian(sv._h, theta, K, None, None, out, None) == 0     # energy, grad and asymmetry may be NULL
        e, g, hs = sv.energy_hessian(theta)
        assert np.array_equal(hs.reshape(-1), out)
        # K = 0: only hess is checked, the energy alone is answered
        sv.set_rotation_program(rx, rz, rc, np.full(len(rx), -1, np.int32), 0, hf, phi0=tied.phi0)
        _refused(sv, INVALID, "hess is NULL", None, 0, None)
        e0 = ctypes.c_double()
        assert sv._L.ovqe_energy_hessian(sv._h, None, 0, ctypes.byref(e0), None, out, None) == 0
        assert e0.value == sv.energy(np.zeros(0)) and sv.energy_hessian(np.zeros(0))[2].shape == (0, 0)
    with SV(n - 1, n_global=1, shard_index=0) as shard:
        _refused(shard, STATE, "shard of a partitioned register", theta, K, out)


def test_workspace_cap_on_a_dense_streaming_case(SV):
    """14 qubits on the streaming path: two stores of 16384 rows x 64 columns x 16 bytes = 32 MiB, 256 slabs and 4 weight records of 64
    doubles, against a cap of 1 MB -> OVQE_ERR_ALLOC naming the bytes; the handle still works afterwards"""
    n, K = 14, 3
    strings = [("YX", [0, 13]), ("XZY", [3, 4, 9]), ("X", [6])]
    xz = [metric_cases.masks.pack_pauli(n, s, q) for s, q in strings]
    rx, rz = np.array([x for x, _ in xz], np.uint64), np.array([z for _, z in xz], np.uint64)
    rc, pidx = np.array([0.7, -0.4, 0.5]), np.arange(3, dtype=np.int32)
    case = Synthetic(n, 5, rx, rz, rc, pidx, None, K, 10, 77)
    theta = np.array([0.3, -0.6, 0.9])
    with SV(n) as sv:
        sv.set_option("force_path", 2)
        sv.set_option("metric_workspace_mb", 1)
        case.load(sv)
        need = hessian_cases.streaming_workspace(n, K, 4)
        assert need == 2 * 16384 * 64 * 16 + 256 * 64 * 8 + 4 * 64 * 8
        _refused(sv, -4, str(need) + " bytes", theta, K, np.zeros(K * K))
        sv.set_option("metric_workspace_mb", 32)
        _refused(sv, -4, str(need) + " bytes", theta, K, np.zeros(K * K))   # the stores alone are exactly 32 MiB
        sv.set_option("metric_workspace_mb", 33)
        _, _, hs, info = _call(sv, theta, 2, case.h1, case.C)
    _compare(hs, case.want(theta), "dense 14-qubit streaming", case.h1, case.C)
    assert info["workspace_bytes"] == need


@pytest.mark.parametrize("path", [0, 2])
def test_energy_and_gradient_are_untouched_by_the_call(SV, h4, path):
    """cached tables stay valid: energy(theta) and energy_batch before and after the call to the bit, energy_gradient unchanged"""
    theta = np.random.default_rng(9).uniform(-0.3, 0.3, h4.K)
    with SV(h4.n) as sv:
        sv.set_option("force_path", path)
        sv.set_hamiltonian(h4.ham)
        sv.set_ucc_program(h4.gens, h4.hf)
        e0 = sv.energy(theta)
        b0 = sv.energy_batch(np.tile(theta, (3, 1)))
        ge0 = sv.energy_gradient(theta)
        sv.energy_hessian(theta)
        assert sv.hessian_info()["path"] == (2 if path == 2 else 1)
        e1 = sv.energy(theta)
        b1 = sv.energy_batch(np.tile(theta, (3, 1)))
        ge1 = sv.energy_gradient(theta)
    assert np.float64(e0).view(np.int64) == np.float64(e1).view(np.int64)
    assert np.array_equal(b0.view(np.int64), b1.view(np.int64))
    # (the compact gradient kernel adds with LDS atomics: it reproduces itself to rounding, with or without a Hessian call in between)
    assert abs(ge0[0] - ge1[0]) <= 1e-13 and np.abs(ge0[1] - ge1[1]).max() <= 1e-13


# ---- optimiser ----------------------------------------------------------------------------------------------------------------------
def test_newton_vqe_on_lih(gpu_lib, lih):
    """LiH UCCSD from theta = 0 through EnergyUCC.newton: at most 1e-8 above L-BFGS-B's energy, the gradient within the tolerance, the
    accepted energies never rise, and the solution is a minimum (lowest Hessian eigenvalue >= -1e-8)"""
    from openvqe_amd.common_files import newton
    from openvqe_amd.evaluator import release_backends
    from openvqe_amd.ucc_family.get_energy_ucc import EnergyUCC

    class Newton(EnergyUCC):
        newton = True

    tol = 1e-6
    release_backends()
    try:
        energies = []
        vqe = Newton()
        res = vqe._minimize(lih.ham, lih.gens, lih.hf, np.zeros(lih.K), energies, "BFGS", tol)
        ev = vqe._evaluator(lih.ham, lih.gens, lih.hf, lih.K)
        assert ev.sv.hessian_info()["path"] == 1
        ref = scipy.optimize.minimize(lambda t: ev.energy_gradient(t), np.zeros(lih.K), jac=True, method="L-BFGS-B")
        low = newton.stability(ev.energy_hessian(res.x)[2])[0]
    finally:
        release_backends()
    print(f"newton: {res.message}; {res.nit} iterations, {res.ncalls} Hessian calls, E = {res.fun:.12f}, max|grad| = {np.abs(res.jac).max():.3e}, "
          f"lowest eigenvalue {low:.3e}; L-BFGS-B: {ref.nit} iterations, E = {ref.fun:.12f}; difference {res.fun - ref.fun:.3e}")
    assert res.fun <= ref.fun + 1e-8
    assert np.abs(res.jac).max() <= tol
    assert np.all(np.diff(res.energies) <= 0.0) and len(energies) == res.ncalls and res.x.shape == (lih.K,)
    assert low >= -1e-8
