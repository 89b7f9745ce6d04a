"""GPU tests of the Fubini-Study metric of the ansatz state (ovqe_metric_tensor: csrc/sv_metric_host.hpp, k_sparse_metric in
csrc/sv_sparse.hpp, csrc/sv_metric.hpp, metric_host.inc; Statevector.metric_tensor / metric_info) against the forward-mode checker of
tests/metric_cases.py, and of natural-gradient VQE (openvqe_amd/common_files/natural_gradient.py, EnergyUCC.natural_gradient).

Tolerance against the checker: |delta g_ij| <= 1e-10 max(1, max_k g_kk), the project's bilinear parity bound.  Every result is also
symmetric to the bit, equal to the bit on a second call, and positive semidefinite within the same bound."""
import ctypes

import numpy as np
import pytest
import scipy.optimize

from openvqe_amd import chem, fermion
from openvqe_amd.backend import compile_ucc_program
from tests import metric_cases

pytestmark = pytest.mark.gpu


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

    def want(self, theta):
        return metric_cases.rotation_metric(self.n, self.hf, self.rx, self.rz, self.rc, self.rp, theta)


@pytest.fixture(scope="module")
def h4():
    return Mol("H4")


@pytest.fixture(scope="module")
def lih():
    return Mol("LiH")


_call, _compare = metric_cases.call_metric, metric_cases.compare


# ---- compact support ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def h4_compact(SV, h4):
    """H4/STO-3G UCCSD, 8 qubits, at random theta and at theta = 0: the compact results the streaming test compares with"""
    theta = np.random.default_rng(8).uniform(-0.3, 0.3, h4.K)
    with SV(h4.n) as sv:
        sv.set_hamiltonian(h4.ham)
        sv.set_ucc_program(h4.gens, h4.hf)
        g, info = _call(sv, theta, 1)
        g0, _ = _call(sv, np.zeros(h4.K), 1)
    return theta, g, g0, info


def test_h4_uccsd_on_the_compact_support(h4, h4_compact):
    theta, g, g0, info = h4_compact
    _compare(g, h4.want(theta), "H4 random theta")
    _compare(g0, h4.want(np.zeros(h4.K)), "H4 theta = 0")
    assert info["tangent_launches"] == 1 and info["gram_launches"] == 1
    assert 0 < info["tangent_amplitudes"] <= 70 and info["store_bytes"] == info["tangent_amplitudes"] * 64 * 8   # the (2, 2) sector of C(8, 4)


def test_lih_uccsd_92_parameters(SV, lih):
    """12 qubits, 92 parameters: two column blocks of the Gram matrix, no Hamiltonian on the handle"""
    assert lih.n == 12 and lih.K == 92
    theta = np.random.default_rng(12).uniform(-0.2, 0.2, lih.K)
    with SV(lih.n) as sv:
        sv.set_ucc_program(lih.gens, lih.hf)
        g, info = _call(sv, theta, 1)
    _compare(g, lih.want(theta), "LiH")
    assert info["tangent_amplitudes"] == 225 and info["store_bytes"] == 225 * 128 * 8


@pytest.fixture(scope="module")
def synth_strings():
    _, gens, hf = fermion.synthetic_molecule(6, 3, 41)
    return gens, hf


@pytest.mark.parametrize("K", [1, 63, 64, 65, 129])
def test_block_edges_of_the_gram_matrix(SV, synth_strings, K):
    """one parameter per rotation, truncated to K: a lone column, a block short of one column, exactly one block, one column into the
    second block (the off-diagonal block pair and its mirror), one column into the third"""
    gens, hf = synth_strings
    n = 12
    rx, rz, rc, rp = metric_cases.one_parameter_per_rotation(gens, n, K)
    theta = np.random.default_rng(K).uniform(-0.4, 0.4, K)
    with SV(n) as sv:
        sv.set_rotation_program(rx, rz, rc, rp, K, hf)
        g, info = _call(sv, theta, 1)
    _compare(g, metric_cases.rotation_metric(n, hf, rx, rz, rc, rp, theta), f"K = {K}")
    assert info["store_bytes"] == info["tangent_amplitudes"] * ((K + 63) // 64 * 64) * 8


@pytest.fixture(scope="module")
def tied_compact(SV):
    n, hf, rx, rz, rc, pidx, phi0, K = metric_cases.tied_program()
    theta = np.random.default_rng(5).uniform(-0.8, 0.8, K)
    with SV(n) as sv:
        sv.set_rotation_program(rx, rz, rc, pidx, K, hf, phi0=phi0)
        g, _ = _call(sv, theta, 1)
    return theta, g


def test_tied_parameter_constant_rotation_and_unused_parameter(tied_compact):
    n, hf, rx, rz, rc, pidx, phi0, K = metric_cases.tied_program()
    theta, g = tied_compact
    _compare(g, metric_cases.rotation_metric(n, hf, rx, rz, rc, pidx, theta, phi0), "tied program")
    assert not g[4].any() and not g[:, 4].any() and g[0, 0] > 0.01


# ---- streaming ----------------------------------------------------------------------------------------------------------------------
def test_streaming_agrees_with_the_compact_path(SV, h4, h4_compact, tied_compact):
    theta, g_compact, _, _ = h4_compact
    with SV(h4.n) as sv:
        sv.set_option("force_path", 2)
        sv.set_ucc_program(h4.gens, h4.hf)
        g, info = _call(sv, theta, 2)
    _compare(g, g_compact, "H4 streaming against compact")
    assert info["tangent_amplitudes"] == 256 and info["store_bytes"] == 256 * 64 * 16 and info["tangent_launches"] >= 2 * len(h4.rx)
    n, hf, rx, rz, rc, pidx, phi0, K = metric_cases.tied_program()
    theta, g_compact = tied_compact
    with SV(n) as sv:
        sv.set_option("force_path", 2)
        sv.set_rotation_program(rx, rz, rc, pidx, K, hf, phi0=phi0)
        g, _ = _call(sv, theta, 2)
    _compare(g, g_compact, "tied program streaming against compact")
    assert not g[4].any() and not g[:, 4].any()


def test_gate_list_literal_frame_and_open_frame(SV):
    """5 qubits, RY / RZ / CNOT with ascale = -2 on a shared parameter, an aconst offset and a leading RZ on a qubit still in |0>:
    literal list, Clifford-frame form, and an open frame (a stray trailing CNOT) give the same metric"""
    n, hf, gates, K = metric_cases.gate_list(False)
    theta = np.random.default_rng(6).uniform(-0.8, 0.8, K)
    want = metric_cases.gate_metric(n, hf, gates, theta)
    assert np.abs(want[0]).max() < 1e-15 and want[1, 1] > 0.1
    got = {}
    for frame, stray in ((1, False), (0, False), (1, True), (0, True)):
        with SV(n) as sv:
            sv.set_option("clifford_frame", frame)
            sv.set_gate_program(metric_cases.gate_list(stray)[2], K, hf)
            literal = sv.program_info()["literal_gates"]
            g, _ = _call(sv, theta, 2)
        assert (literal > 0) == (frame == 0), (frame, stray, literal)
        _compare(g, want, f"gate list clifford_frame = {frame}, stray CNOT = {stray}")
        assert np.abs(g[0]).max() <= metric_cases.bound(want) and np.abs(g[:, 0]).max() <= metric_cases.bound(want)
        got[(frame, stray)] = g
    for g in got.values():
        assert np.abs(g - got[(1, False)]).max() <= metric_cases.bound(want)


# ---- contract -----------------------------------------------------------------------------------------------------------------------
def _refused(sv, rc_want, text, theta, K, out):
    rc = sv._L.ovqe_metric_tensor(sv._h, theta, K, out)
    msg = (sv._L.ovqe_last_error(sv._h) or b"").decode()
    assert rc == rc_want and text in msg, (rc, msg)


def test_refusals(SV):
    INVALID, ALLOC, STATE = -1, -4, -5
    n, hf, rx, rz, rc, pidx, phi0, K = metric_cases.tied_program()
    theta, out = np.zeros(K), np.zeros(K * K)
    with SV(n) as sv:
        info = (ctypes.c_int64 * 9)(*([7] * 9))
        assert sv._L.ovqe_metric_info(sv._h, info, 9) == 0 and not any(info)            # zeros before the first call
        info = (ctypes.c_int64 * 11)(*([7] * 11))
        assert sv._L.ovqe_metric_info(sv._h, info, 11) == 0 and not any(info)           # ... the tangent form and its LDS bytes included
        _refused(sv, STATE, "no program set", theta, K, out)
        sv.set_rotation_program(rx, rz, rc, pidx, K, hf, phi0=phi0)
        _refused(sv, INVALID, "K = 4", theta, K - 1, out)
        _refused(sv, INVALID, "theta is NULL", None, K, out)
        _refused(sv, INVALID, "metric is NULL", theta, K, None)
        sv.set_option("real_state", 1)
        _refused(sv, STATE, "real_state", theta, K, out)
        sv.set_option("real_state", 0)
        assert sv.metric_tensor(theta).shape == (K, K)
        # K = 0: only metric is checked
        sv.set_rotation_program(rx, rz, rc, np.full(len(rx), -1, np.int32), 0, hf, phi0=phi0)
        _refused(sv, INVALID, "metric is NULL", None, 0, None)
        assert sv._L.ovqe_metric_tensor(sv._h, None, 0, out) == 0
        assert sv.metric_tensor(np.zeros(0)).shape == (0, 0)
    with SV(n - 1, n_global=1, shard_index=0) as shard:
        _refused(shard, STATE, "shard of a partitioned register", theta, K, out)


def test_workspace_cap_on_a_dense_streaming_case(SV):
    """14 qubits on the streaming path: 16384 rows x 64 columns x 16 bytes = 16 MiB of tangent store against a cap of 1 MB ->
    OVQE_ERR_ALLOC naming the bytes; the handle still works afterwards"""
    n, K = 14, 3
    strings = [("YX", [0, 13]), ("XZY", [3, 4, 9]), ("X", [6])]
    xz = [metric_cases.masks.pack_pauli(n, s, q) for s, q in strings]
    rx, rz = np.array([x for x, _ in xz], np.uint64), np.array([z for _, z in xz], np.uint64)
    rc, pidx = np.array([0.7, -0.4, 0.5]), np.arange(3, dtype=np.int32)
    theta = np.array([0.3, -0.6, 0.9])
    with SV(n) as sv:
        sv.set_option("force_path", 2)
        sv.set_option("metric_workspace_mb", 1)
        sv.set_rotation_program(rx, rz, rc, pidx, K, 5)
        _refused(sv, -4, str(16384 * 64 * 16) + " bytes", theta, K, np.zeros(K * K))
        sv.set_option("metric_workspace_mb", 16)
        g, info = _call(sv, theta, 2)
    _compare(g, metric_cases.rotation_metric(n, 5, rx, rz, rc, pidx, theta), "dense 14-qubit streaming")
    assert info["store_bytes"] == 16384 * 64 * 16 and info["tangent_launches"] == 6


@pytest.mark.parametrize("path", [0, 2])
def test_energy_and_gradient_are_untouched_by_the_call(SV, h4, path):
    """cached tables stay valid: energy(theta) before and after the call to the bit, energy_gradient unchanged"""
    theta = np.random.default_rng(9).uniform(-0.3, 0.3, h4.K)
    with SV(h4.n) as sv:
        sv.set_option("force_path", path)
        sv.set_hamiltonian(h4.ham)
        sv.set_ucc_program(h4.gens, h4.hf)
        e0 = sv.energy(theta)
        b0 = sv.energy_batch(np.tile(theta, (3, 1)))
        ge0 = sv.energy_gradient(theta)
        sv.metric_tensor(theta)
        assert sv.metric_info()["path"] == (2 if path == 2 else 1)
        e1 = sv.energy(theta)
        b1 = sv.energy_batch(np.tile(theta, (3, 1)))
        ge1 = sv.energy_gradient(theta)
    assert np.float64(e0).view(np.int64) == np.float64(e1).view(np.int64)
    assert np.array_equal(b0.view(np.int64), b1.view(np.int64))
    # (the compact gradient kernel adds with LDS atomics: it reproduces itself to rounding, with or without a metric call in between)
    assert abs(ge0[0] - ge1[0]) <= 1e-13 and np.abs(ge0[1] - ge1[1]).max() <= 1e-13


# ---- optimiser ----------------------------------------------------------------------------------------------------------------------
def test_natural_gradient_vqe_on_lih(gpu_lib, lih):
    """LiH UCCSD from theta = 0 through EnergyUCC.natural_gradient: the energy never rises and ends at most 1e-8 above L-BFGS-B's"""
    from openvqe_amd.evaluator import release_backends
    from openvqe_amd.ucc_family.get_energy_ucc import EnergyUCC

    class Natural(EnergyUCC):
        natural_gradient = True

    release_backends()
    try:
        energies = []
        vqe = Natural()
        res = vqe._minimize(lih.ham, lih.gens, lih.hf, np.zeros(lih.K), energies, "BFGS", 1e-6)
        ev = vqe._evaluator(lih.ham, lih.gens, lih.hf, lih.K)
        assert ev.sv.metric_info()["path"] == 1
        ref = scipy.optimize.minimize(lambda t: ev.energy_gradient(t), np.zeros(lih.K), jac=True, method="L-BFGS-B")
    finally:
        release_backends()
    print(f"natural gradient: {res.message}; {res.nit} steps, {res.nfev} gradients, E = {res.fun:.12f}; L-BFGS-B: {ref.nit} iterations, "
          f"E = {ref.fun:.12f}; difference {res.fun - ref.fun:.3e}")
    assert np.all(np.diff(res.energies) <= 0.0) and len(res.energies) == res.nit + 1
    assert len(energies) == res.nfev and res.x.shape == (lih.K,)
    assert res.fun <= ref.fun + 1e-8
