"""GPU tests of the Fubini-Study metric's tangent kernels AT THEIR BOUNDARIES (k_sparse_metric<true / false> in csrc/sv_sparse.hpp,
k_metric_sweep / k_metric_add in csrc/sv_metric.hpp, the choice between them in csrc/metric_host.inc): a support of exactly
metric::MAX_SUPPORT = 4096 states with compact index 4095 in the 12-bit fields of the pair words, the last program whose tables are staged
in LDS and the first whose tables stay in global memory, the last program that fits a workgroup's LDS budget and the first that streams
although a compact program exists, the refusal one qubit beyond the cap, the pattern-table / plain-rotation boundary at x weight 7 | 8 and
a constant inside a same-x run, the streaming kernels over more than one block of 64 columns, over more row pairs than the grid holds
workgroups, and the literal gates on every bit position of a 10-qubit register.

Every case goes through metric_cases.call_metric (symmetric to the bit, the same bits on a second call, positive semidefinite within the
bound) and is compared with the forward-mode checker of tests/metric_cases.py within metric_cases.bound, |delta g_ij| <= 1e-10 max(1,
max_k g_kk).  Which kernel form ran is read from metric_info()["tangent_form"] / ["tangent_lds_bytes"] and compared with the formula of
sp_metric_lds restated in metric_cases.tangent_lds_bytes."""
import numpy as np
import pytest

from openvqe_amd import fermion
from tests import metric_cases

pytestmark = pytest.mark.gpu

call, compare = metric_cases.call_metric, metric_cases.compare


@pytest.fixture(scope="module")
def SV(gpu_lib):
    from openvqe_amd.backend import Statevector
    return Statevector


def _timing(what, info):
    print(f"{what}: tangents {info['tangents_us']} us, Gram {info['gram_us']} us, finish {info['finish_us']} us, "
          f"{info['tangent_launches']} tangent launches, form {info['tangent_form']}, LDS {info['tangent_lds_bytes']} bytes")


# ---- the compact kernel at the support cap: staged | unstaged | does not fit ----------------------------------------------------------
CUBE_K = 6
# R: npairs, staged bytes, unstaged bytes, form (1 staged, 2 unstaged, 0 streaming) of cube_program(12, R, 6), from the host planner
CUBE_TABLE = {20: (20479, 148252, 66016, 1), 21: (22527, 156492, 66048, 2), 3669: (7493631, None, 153600, 2), 3670: (7495679, None, 153616, 0)}
_cube_memo = {}


def _cube(n, R):
    """program, theta and the checker's metric of cube_program(n, R, 6, 100 + R) (the seed tests/test_metric_cases.py checks), once"""
    if (n, R) not in _cube_memo:
        prog = metric_cases.cube_program(n, R, CUBE_K, 100 + R)
        theta = np.random.default_rng(R).uniform(-0.8, 0.8, CUBE_K)
        _, hf, rx, rz, rc, pidx, phi0, _ = prog
        want = metric_cases.rotation_metric(n, hf, rx, rz, rc, pidx, theta, phi0)
        assert np.max(np.diag(want)) <= 4.0
        want.setflags(write=False)
        _cube_memo[(n, R)] = (prog, theta, want, {})
    return _cube_memo[(n, R)]


def _cube_gpu(SV, n, R, force):
    """(g, info) of the cube program on the path the library chooses (force = 0) or on the streaming path (force = 2), once"""
    prog, theta, want, got = _cube(n, R)
    if force not in got:
        _, hf, rx, rz, rc, pidx, phi0, K = prog
        compact, _ = metric_cases.tangent_form(*metric_cases.cube_sizes(n, R)) if n <= 12 else (0, 0)
        with SV(n) as sv:
            if force:
                sv.set_option("force_path", force)
            sv.set_rotation_program(rx, rz, rc, pidx, K, hf, phi0=phi0)
            got[force] = call(sv, theta, 1 if compact and not force else 2)
        _timing(f"cube_program({n}, {R}) force_path = {force}", got[force][1])
    return got[force]


@pytest.mark.parametrize("R", [20, 21, 3669, 3670])
def test_compact_forms_at_the_support_cap(SV, R):
    """4096 states, compact index 4095 in both fields of the pair words, mpad = 4096 (64 KiB of psi and tangent): R = 20 is the last program
    whose op records and pair words are staged in LDS, 21 the first that reads them from global memory, 3669 the last whose angle table
    fits (its LDS bytes EQUAL the budget of 150 KiB), 3670 streams although a compact program exists"""
    n = 12
    npairs, staged, unstaged, form = CUBE_TABLE[R]
    m, ntab, nops, np_ = metric_cases.cube_sizes(n, R)
    assert (m, ntab, nops, np_) == (metric_cases.MAX_SUPPORT, R, R, npairs)
    assert metric_cases.tangent_lds_bytes(m, ntab, nops, np_, False) == unstaged
    assert staged is None or metric_cases.tangent_lds_bytes(m, ntab, nops, np_, True) == staged
    lds = {1: staged, 2: unstaged, 0: 0}[form]
    assert metric_cases.tangent_form(m, ntab, nops, np_) == (form, lds)
    g, info = _cube_gpu(SV, n, R, 0)
    assert info["path"] == (1 if form else 2) and info["tangent_form"] == form and info["tangent_lds_bytes"] == lds, info
    assert info["tangent_amplitudes"] == 4096
    if form:
        assert info["store_bytes"] == 4096 * 64 * 8 and info["tangent_launches"] == 1
    else:
        assert info["path"] == 2 and info["store_bytes"] == 4096 * 64 * 16 and info["tangent_launches"] >= R
    compare(g, _cube(n, R)[2], f"cube_program(12, {R}) form {form}")


@pytest.mark.parametrize("R", [20, 21, 3669])
def test_compact_forms_agree_with_streaming(SV, R):
    """the same programs under force_path = 2: the staged (20) and the unstaged (21, 3669) compact results agree with the streaming
    kernels' and both with the checker"""
    n = 12
    g, _ = _cube_gpu(SV, n, R, 0)
    gs, info = _cube_gpu(SV, n, R, 2)
    assert info["tangent_form"] == 0 and info["tangent_lds_bytes"] == 0 and info["tangent_amplitudes"] == 4096
    want = _cube(n, R)[2]
    compare(gs, want, f"cube_program(12, {R}) streaming")
    compare(g, gs, f"cube_program(12, {R}) compact against streaming")


def test_one_qubit_beyond_the_support_cap_streams(SV):
    """the same builder on 13 qubits reaches 8192 states: build_compact declines at state 4097 and the call streams"""
    n, R = 13, 21
    g, info = _cube_gpu(SV, n, R, 0)
    assert info["path"] == 2 and info["tangent_form"] == 0 and info["tangent_lds_bytes"] == 0
    assert info["tangent_amplitudes"] == 8192 and info["store_bytes"] == 8192 * 64 * 16
    compare(g, _cube(n, R)[2], "cube_program(13, 21)")


# ---- pattern table | plain rotation ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [7, 8])
def test_table_op_boundary_and_constant_inside_a_run(SV, w):
    """x weight 7: the widest rotation fused into a pattern table (64 patterns, pattern index 63 in the pair words); weight 8: the first
    that stays a plain rotation; behind it a same-x run with a constant between two parameters.  The LDS bytes tell the two apart: they
    count the table entries."""
    n, hf, rx, rz, rc, pidx, phi0, K, heavy = metric_cases.weight_program(12, w)
    theta = np.random.default_rng(w).uniform(-0.8, 0.8, K)
    want = metric_cases.rotation_metric(n, hf, rx, rz, rc, pidx, theta, phi0)
    m, ntab, nops, npairs = metric_cases.weight_sizes(w)
    assert ntab - nops == (63 if w == 7 else 0)
    with SV(n) as sv:
        sv.set_rotation_program(rx, rz, rc, pidx, K, hf, phi0=phi0)
        g, info = call(sv, theta, 1)
    assert info["tangent_form"] == 1 and info["tangent_amplitudes"] == m, info
    assert info["tangent_lds_bytes"] == metric_cases.tangent_lds_bytes(m, ntab, nops, npairs, True), info
    with SV(n) as sv:
        sv.set_option("force_path", 2)
        sv.set_rotation_program(rx, rz, rc, pidx, K, hf, phi0=phi0)
        gs, infos = call(sv, theta, 2)
    assert infos["tangent_form"] == 0
    compare(g, want, f"weight_program(12, {w})")
    compare(gs, want, f"weight_program(12, {w}) streaming")
    compare(g, gs, f"weight_program(12, {w}) compact against streaming")
    assert np.all(np.diag(g) > 0.01)


# ---- streaming: column blocks ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def h4_strings():
    """the UCCSD strings of four orbitals and two pairs on 8 qubits (160 rotations), from the Hartree-Fock determinant"""
    return fermion.uccsd_generators(4, 2), 0b11110000


def _stream_and_compact(SV, n, hf, rx, rz, rc, pidx, K, theta, what):
    want = metric_cases.rotation_metric(n, hf, rx, rz, rc, pidx, theta)
    with SV(n) as sv:
        sv.set_option("force_path", 2)
        sv.set_rotation_program(rx, rz, rc, pidx, K, hf)
        g, info = call(sv, theta, 2)
    wpad = (K + 1 + 63) // 64 * 64
    assert info["tangent_form"] == 0 and info["tangent_amplitudes"] == 256 and info["store_bytes"] == 256 * wpad * 16, info
    assert info["tangent_launches"] == 2 * len(rx)
    with SV(n) as sv:
        sv.set_rotation_program(rx, rz, rc, pidx, K, hf)
        gc, _ = call(sv, theta, 1)
    compare(g, want, f"{what} streaming")
    compare(gc, want, f"{what} compact")
    compare(g, gc, f"{what} streaming against compact")
    return g


@pytest.mark.parametrize("K", [63, 64, 65, 128, 129])
def test_streaming_column_blocks(SV, h4_strings, K):
    """store widths 64, 65, 66, 129, 130 (psi is column 0): one block of k_metric_sweep's second grid dimension, one column into the
    second, the second block's edge and one column into the third — whole waves beyond the live columns, and the complex Gram kernel on
    more than one block pair"""
    gens, hf = h4_strings
    rx, rz, rc, pidx = metric_cases.one_parameter_per_rotation(gens, 8, K)
    theta = np.random.default_rng(K).uniform(-0.4, 0.4, K)
    g = _stream_and_compact(SV, 8, hf, rx, rz, rc, pidx, K, theta, f"K = {K}")
    assert np.all(np.diag(g) > 1e-4)


def test_streaming_last_parameter_met_first(SV, h4_strings):
    """parameter K - 1 on the first rotation, 0..K-2 behind it: the live column count jumps to K + 1 at once and the sweeps run over the
    zero columns of two blocks"""
    gens, hf = h4_strings
    K = 65
    rx, rz, rc, _ = metric_cases.one_parameter_per_rotation(gens, 8, K)
    pidx = np.concatenate([[K - 1], np.arange(K - 1)]).astype(np.int32)
    theta = np.random.default_rng(K + 1000).uniform(-0.4, 0.4, K)
    _stream_and_compact(SV, 8, hf, rx, rz, rc, pidx, K, theta, "last parameter first")


# ---- streaming: more rows than the grid holds workgroups ------------------------------------------------------------------------------
def test_streaming_grid_cap_on_19_qubits(SV):
    """2^18 row pairs ask for 65536 workgroups of four and get 65535: the smallest register on which k_metric_sweep's stride loop runs a
    second time, in the pair form and (2^19 rows) in the diagonal form.  Five rotations: pivot bit 18, pivot bit 0 (x = 1), a diagonal
    string (k_metric_add with x = 0), a constant and a string on every qubit.  From |hf> = |1...1> the amplitudes sit in the LAST row
    pairs of each sweep — the ones only the second turn of the stride loop reaches — and the constant's x, all bits but 18 and 0, closes
    the eight-state support under the full-weight string, so that g_22 and g_02 depend on every angle and on the diagonal's phases"""
    n, K = 19, 3
    top, full = 1 << 18, (1 << 19) - 1
    rng = np.random.default_rng(21)
    zc, zf = int(rng.integers(1, full)), int(rng.integers(1, full))
    rx = np.array([top, 1, 0, full ^ top ^ 1, full], np.uint64)
    rz = np.array([top | 1 << 7, top | 1 << 9 | 1, top | 1 << 11 | 1 << 3, zc, zf], np.uint64)
    rc = np.array([0.7, -0.5, 0.4, 1.0, 0.9])
    pidx = np.array([0, 1, 0, -1, 2], np.int32)
    phi0 = np.array([0.0, 0.2, -0.3, 0.6, 0.0])
    theta = np.array([0.3, -0.7, 0.5])
    want = metric_cases.rotation_metric(n, full, rx, rz, rc, pidx, theta, phi0)
    with SV(n) as sv:
        sv.set_option("force_path", 2)
        sv.set_rotation_program(rx, rz, rc, pidx, K, full, phi0=phi0)
        g, info = call(sv, theta, 2)
    _timing("19 qubits", info)
    assert info["tangent_form"] == 0 and info["tangent_amplitudes"] == 1 << 19 and info["store_bytes"] == (1 << 19) * 64 * 16
    assert info["tangent_launches"] == 5 + 4
    compare(g, want, "19 qubits streaming")
    assert np.all(np.diag(want) > 0.01) and abs(want[0, 2]) > 0.01 and want[2, 2] < 0.8   # (0.81 = coeff^2 where <P> vanishes)


# ---- streaming: literal gates on every bit position -----------------------------------------------------------------------------------
def test_wide_gate_list_literal_frame_and_open_frame(SV):
    """10 qubits, all six gates: H and X on the top and the bottom bit, CNOT with the control above and below the target, adjacent and far
    apart, on 1024 amplitudes; literal list, Clifford-frame form and an open frame give the same metric"""
    n, hf, gates, K = metric_cases.wide_gate_list(False)
    theta = np.random.default_rng(10).uniform(-0.8, 0.8, K)
    want = metric_cases.gate_metric(n, hf, gates, theta)
    got = {}
    for frame, stray in ((1, False), (0, False), (1, True), (0, True)):
        with SV(n) as sv:
            sv.set_option("clifford_frame", frame)
            sv.set_gate_program(metric_cases.wide_gate_list(stray)[2], K, hf)
            literal = sv.program_info()["literal_gates"]
            g, info = call(sv, theta, 2)
        assert (literal > 0) == (frame == 0), (frame, stray, literal)
        assert info["tangent_form"] == 0 and info["tangent_amplitudes"] == 1024 and info["store_bytes"] == 1024 * 64 * 16
        compare(g, want, f"wide gate list clifford_frame = {frame}, stray gates = {stray}")
        got[(frame, stray)] = g
    for g in got.values():
        assert np.abs(g - got[(1, False)]).max() <= metric_cases.bound(want)
    assert np.all(np.diag(want) > 0.01)
