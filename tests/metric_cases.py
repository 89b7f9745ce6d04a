"""TEST INFRASTRUCTURE ONLY — exact forward-mode checker of the Fubini-Study metric (ovqe_metric_tensor) and the case lists of
tests/test_metric_cases.py / tests/test_gpu_metric.py / tests/test_gpu_metric_edges.py, with the checks every GPU result gets.

The checker carries psi and the LIVE tangents T_k = d psi / d theta_k (rows of a matrix) through the program with
``oracle.masks.rotate`` / the gate functions, and behind every parameterised rotation adds coeff (-i P) psi to its tangent with
``oracle.masks.apply_pauli_sum``: no finite differences.  g = Re(<T_i|T_j> - <T_i|psi><psi|T_j>)."""
import numpy as np

from oracle import dense, masks


def metric_of(psi, T):
    """g from the state and the (K, 2^n) matrix of its tangents"""
    G = T.conj() @ T.T
    a = T.conj() @ psi          # a_i = <T_i|psi>
    return (G - np.outer(a, a.conj())).real


def _angle(c, c0, p, theta):
    return float(c0) + (float(c) * float(theta[p]) if p >= 0 else 0.0)


def rotation_tangents(n, hf, rx, rz, rc, pidx, theta, phi0=None):
    """(psi, T) of prod_r exp(-i (rc_r theta[pidx_r] + phi0_r) P_r)|hf>, rotation 0 first; T is (len(theta), 2^n)"""
    K = len(theta)
    psi = np.zeros(1 << n, np.complex128)
    psi[int(hf)] = 1.0
    T = np.zeros((K, 1 << n), np.complex128)
    live = []
    phi0 = np.zeros(len(rx)) if phi0 is None else phi0
    for x, z, c, c0, p in zip(rx, rz, rc, phi0, pidx):
        x, z, p = int(x), int(z), int(p)
        phi = _angle(c, c0, p, theta)
        psi = masks.rotate(psi, x, z, phi)
        for k in live:
            T[k] = masks.rotate(T[k], x, z, phi)
        if p >= 0:
            if p not in live:
                live.append(p)
            T[p] += masks.apply_pauli_sum(psi, [x], [z], [-1j * float(c)])
    return psi, T


def rotation_metric(n, hf, rx, rz, rc, pidx, theta, phi0=None):
    return metric_of(*rotation_tangents(n, hf, rx, rz, rc, pidx, theta, phi0))


_AXIS = {"RX": "X", "RY": "Y", "RZ": "Z"}


def gate_tangents(n, hf, gates, theta):
    """(psi, T) of a literal gate list [(name, qubits, angle_scale, angle_const, param or -1)]: RX / RY / RZ(a) = exp(-i a P / 2)"""
    K = len(theta)
    psi = np.zeros(1 << n, np.complex128)
    psi[int(hf)] = 1.0
    T = np.zeros((K, 1 << n), np.complex128)
    for name, qubits, scale, const, p in gates:
        if name in _AXIS:
            x, z = masks.pack_pauli(n, _AXIS[name], [qubits[0]])
            phi = 0.5 * _angle(scale, const, p, theta)
            psi = masks.rotate(psi, x, z, phi)
            for k in range(K):
                T[k] = masks.rotate(T[k], x, z, phi)
            if p >= 0:
                T[p] += masks.apply_pauli_sum(psi, [x], [z], [-0.5j * float(scale)])
        elif name == "CNOT":
            psi = masks.gate_cnot(psi, n, qubits[0], qubits[1])
            for k in range(K):
                T[k] = masks.gate_cnot(T[k], n, qubits[0], qubits[1])
        else:
            m = dense.gate_matrix(name, 0.0)
            psi = masks.gate_1q(psi, n, qubits[0], m)
            for k in range(K):
                T[k] = masks.gate_1q(T[k], n, qubits[0], m)
    return psi, T


def gate_metric(n, hf, gates, theta):
    return metric_of(*gate_tangents(n, hf, gates, theta))


# ---- cases --------------------------------------------------------------------------------------------------------------------------
def tied_program(n=6):
    """a real program (odd-Y strings) with parameter 0 tied across NON-ADJACENT rotations, a constant-angle rotation (pidx < 0), an
    offset, and a trailing parameter no rotation uses -> (n, hf, rx, rz, rc, pidx, phi0, K)"""
    strings = [("YX", [0, 2]), ("XY", [1, 3]), ("YXXX", [0, 1, 2, 3]), ("XY", [0, 2]), ("YZX", [2, 3, 4]), ("XXXY", [0, 1, 4, 5]),
               ("YX", [1, 3]), ("XZY", [3, 4, 5])]
    pidx = [0, 1, 2, 0, -1, 3, 1, 0]
    rc = [0.7, -0.4, 1.0, -0.35, 1.0, 0.5, 0.9, 0.25]
    phi0 = [0.0, 0.1, 0.0, 0.0, 0.37, 0.0, -0.2, 0.0]
    xz = [masks.pack_pauli(n, s, q) for s, q in strings]
    rx = np.array([x for x, _ in xz], np.uint64)
    rz = np.array([z for _, z in xz], np.uint64)
    hf = int("110100"[:n].ljust(n, "0"), 2)
    return n, hf, rx, rz, np.array(rc), np.array(pidx, np.int32), np.array(phi0), 5


def gate_list(stray_cnot=False):
    """5 qubits, RY / RZ / CNOT: a leading RZ on a qubit still in |0> (parameter 0: a zero row), ascale = -2 on the shared parameter 1,
    an aconst offset; the CNOTs cancel in pairs (a closed Clifford frame); ``stray_cnot``: a trailing CNOT that leaves the frame open
    -> (n, hf, gates, K)"""
    g = [("RZ", [0], 1.0, 0.0, 0),
         ("RY", [0], 1.0, 0.3, 1), ("RY", [1], -2.0, 0.0, 1), ("CNOT", [0, 1], 0.0, 0.0, -1),
         ("RZ", [1], 1.0, -0.4, 2), ("RY", [2], 0.8, 0.0, 3), ("CNOT", [0, 1], 0.0, 0.0, -1),
         ("CNOT", [1, 2], 0.0, 0.0, -1), ("RY", [3], 1.0, 0.9, -1), ("RZ", [2], -2.0, 0.0, 1), ("CNOT", [1, 2], 0.0, 0.0, -1),
         ("RY", [4], 1.0, 0.0, 4), ("RY", [2], 1.0, 0.0, 2)]
    if stray_cnot:
        g.append(("CNOT", [0, 4], 0.0, 0.0, -1))
    return 5, 0, g, 5


def one_parameter_per_rotation(generators, nbqbits, K):
    """the strings of ``generators`` as a program with its own parameter for every rotation, truncated to K rotations"""
    from openvqe_amd.backend import compile_ucc_program
    rx, rz, rc, _, _ = compile_ucc_program(nbqbits, generators)
    assert len(rx) >= K
    return rx[:K], rz[:K], rc[:K], np.arange(K, dtype=np.int32)


def bound(g):
    """the project's bilinear parity bound on |delta g_ij|"""
    return 1e-10 * max(1.0, float(np.max(np.diag(g))) if g.size else 1.0)


# ---- the checks every GPU result gets -------------------------------------------------------------------------------------------------
def call_metric(sv, theta, path):
    """the metric twice, with the checks every result gets -> (g, info)"""
    g = sv.metric_tensor(theta)
    info = sv.metric_info()
    again = sv.metric_tensor(theta)
    K = len(theta)
    assert g.shape == (K, K) and g.dtype == np.float64
    assert np.array_equal(g, g.T)
    assert np.array_equal(g.view(np.int64), again.view(np.int64))
    assert info["path"] == path and info["K"] == K, info
    if K:
        low = np.linalg.eigvalsh(g)[0]
        print(f"path {path} K {K} smallest eigenvalue {low:.3e} info {info}")
        assert low >= -bound(g)
    return g, info


def compare(g, want, what):
    err = np.abs(g - want).max() if g.size else 0.0
    print(f"{what}: max|delta g| = {err:.3e}, bound {bound(want):.3e}, max g_kk = {np.max(np.diag(want)) if g.size else 0:.4f}")
    assert err <= bound(want)


# ---- boundary cases of the tangent kernels (tests/test_gpu_metric_edges.py, tests/cpu/metric_plan_check.cpp boundary) ----------------
LDS_WG_BUDGET = 150 * 1024   # what metric_host.inc compares the tangent kernel's dynamic LDS with
MAX_SUPPORT = 4096           # metric::MAX_SUPPORT


def tangent_lds_bytes(m, ntab, nops, npairs, stage):
    """sp_metric_lds (csrc/sv_sparse.hpp): psi and the tangent ([mpad] doubles each), cos / sin and the derivative coefficient per table
    entry; staged: the 16-byte op records and the 4-byte pair words behind them"""
    mpad = (m + 1) & ~1
    base = 2 * mpad * 8 + ntab * 16 + ((ntab + 1) & ~1) * 8
    return base + nops * 16 + npairs * 4 if stage else base


def tangent_form(m, ntab, nops, npairs):
    """(form, LDS bytes) the way run_metric chooses: 1 staged, 2 unstaged, 0 streaming although a compact program exists"""
    staged, plain = tangent_lds_bytes(m, ntab, nops, npairs, True), tangent_lds_bytes(m, ntab, nops, npairs, False)
    if staged <= LDS_WG_BUDGET:
        return 1, staged
    return (2, plain) if plain <= LDS_WG_BUDGET else (0, 0)


def cube_sizes(n, R):
    """(m, ntab, nops, npairs) of cube_program(n, R, ...): every rotation its own op and table entry, rotation r < n pairs the 2^r
    states reached so far with 2^r new ones, every later one the whole register"""
    return 1 << n, R, R, (1 << n) - 1 + (R - n) * (1 << (n - 1))


def cube_program(n, R, K, seed):
    """a real program whose support is the whole register: rotations 0..n-1 are a single Y on qubit r (the support doubles each time),
    the others random odd-Y strings of weight 2..5; EVERY rotation has an offset (no run is fused into a pattern table: one op, one table
    entry and |S| / 2 pairs per rotation), pidx is drawn from -1..K-1 (each value at least once), and the coefficients shrink with the rotations per parameter so
    that max g_kk stays below 4 (a random walk of R / (K + 1) steps) -> (n, hf, rx, rz, rc, pidx, phi0, K)"""
    assert R >= n
    rng = np.random.default_rng(seed)
    strings = [("Y", [r]) for r in range(n)]
    for _ in range(n, R):
        w = int(rng.integers(2, 6))
        qubits = sorted(int(q) for q in rng.choice(n, w, replace=False))
        while True:
            letters = "".join(rng.choice(list("XYZ"), w))
            if letters.count("Y") & 1:
                break
        strings.append((letters, qubits))
    xz = [masks.pack_pauli(n, s, q) for s, q in strings]
    rx = np.array([x for x, _ in xz], np.uint64)
    rz = np.array([z for _, z in xz], np.uint64)
    pidx = rng.integers(-1, K, R).astype(np.int32)
    if R > K:   # ... every value at least once
        pidx[:K + 1] = rng.permutation(np.arange(-1, K))
    phi0 = rng.uniform(0.2, 1.0, R) * rng.choice([-1.0, 1.0], R)
    rc = rng.uniform(0.3, 1.0, R) * rng.choice([-1.0, 1.0], R) * min(0.6, 1.2 / np.sqrt(R / (K + 1.0)))
    hf = int(rng.integers(1, 1 << n))
    return n, hf, rx, rz, rc, pidx, phi0, K


def weight_sizes(w):
    """(m, ntab, nops, npairs) of weight_program(n, w): w + 1 single-Y rotations, the weight-w rotation — a pattern table of 2^(w-1)
    entries up to w = 7, one plain entry from w = 8 on — and the run of three, whose x holds a new qubit"""
    m = 1 << (w + 2)
    return m, (w + 1) + (1 << (w - 1) if w <= 7 else 1) + 3, (w + 1) + 1 + 3, (1 << (w + 1)) - 1 + (1 << w) + 3 * (m >> 1)


def weight_program(n, w):
    """single-Y rotations (with offsets) on qubits 0..w populate every pattern of ONE parameterised rotation of weight w without offset —
    X / Y on qubits 0..w-1, Z on qubit w — which try_table_op fuses into a pattern table up to w = 7 and leaves a plain rotation from
    w = 8 on; behind it a same-x run of three strings on qubits (1, w, w + 1) whose middle one is a constant (pidx = -1) and whose outer
    two carry different parameters: never fused -> (n, hf, rx, rz, rc, pidx, phi0, K, heavy) with ``heavy`` the index of the weight-w
    rotation (the run is heavy + 1 .. heavy + 3)"""
    assert 3 <= w and w + 2 <= n
    strings = [("Y", [q]) for q in range(w + 1)]
    pidx = [q % 2 for q in range(w + 1)]
    rc = [0.35 + 0.05 * q for q in range(w + 1)]
    phi0 = [0.3 - 0.11 * q if q != 2 else 0.7 for q in range(w + 1)]
    heavy = len(strings)
    strings.append(("Y" + "X" * (w - 3) + "YY" + "Z", list(range(w + 1))))
    pidx.append(2)
    rc.append(0.8)
    phi0.append(0.0)
    run = (1, w, w + 1)
    strings += [("ZXYX", [0, *run]), ("YXX", list(run)), ("XXYZ", [*run, n - 1] if n - 1 > w + 1 else list(run))]
    pidx += [3, -1, 0]
    rc += [-0.6, 1.0, 0.45]
    phi0 += [0.0, 0.37, 0.0]
    xz = [masks.pack_pauli(n, s, q) for s, q in strings]
    rx = np.array([x for x, _ in xz], np.uint64)
    rz = np.array([z for _, z in xz], np.uint64)
    hf = (1 << (n - 1)) | 5
    return n, hf, rx, rz, np.array(rc), np.array(pidx, np.int32), np.array(phi0), 4, heavy


def wide_gate_list(stray=False, n=10):
    """all six gates on a register wide enough for every bit position: H and X on qubit 0 and on qubit n-1, CNOT with the control index
    above and below the target on adjacent and far-apart qubits, RZ and RY on the top and the bottom qubit, RX in between; 5 parameters,
    parameter 1 shared with ascale = -2, one aconst offset.  The Clifford gates come back in reverse order (a closed frame: each is its
    own inverse); ``stray``: a trailing CNOT and H leave the frame open -> (n, hf, gates, K)"""
    t, b = 0, n - 1
    cliff = [("H", [t]), ("X", [b]), ("CNOT", [3, 4]), ("CNOT", [7, 6]), ("CNOT", [t, b]), ("H", [b]), ("X", [t]), ("CNOT", [b, t]),
             ("CNOT", [8, 2]), ("CNOT", [1, 5])]
    rot_a = [("RY", [t], 1.0, 0.3, 0), ("RZ", [b], 1.0, 0.0, 1), ("RX", [4], 0.7, 0.0, 2), ("RY", [b], -2.0, 0.0, 1), ("RZ", [t], 1.0, -0.4, 3),
             ("RX", [6], 1.0, 0.0, 4), ("RY", [2], 0.9, 0.0, 0), ("RZ", [5], 1.0, 0.0, 2), ("RY", [7], 1.0, 0.9, -1), ("RX", [t], 1.0, 0.0, 3)]
    rot_b = [("RY", [5], 1.0, 0.0, 4), ("RZ", [2], -2.0, 0.0, 1), ("RX", [b], 0.8, 0.0, 3), ("RY", [t], 1.0, 0.0, 2), ("RZ", [b], 1.0, 0.0, 4),
             ("RY", [6], 1.0, 0.0, 0), ("RX", [3], 1.0, 0.2, 2), ("RZ", [4], 0.6, 0.0, 3), ("RY", [b], 1.0, 0.0, 4), ("RZ", [t], 1.0, 0.0, 0)]
    g = []
    for (name, qubits), r in zip(cliff, rot_a):
        g += [(name, qubits, 0.0, 0.0, -1), r]
    for (name, qubits), r in zip(reversed(cliff), rot_b):
        g += [(name, qubits, 0.0, 0.0, -1), r]
    if stray:
        g += [("CNOT", [b, 1], 0.0, 0.0, -1), ("H", [t], 0.0, 0.0, -1)]
    hf = (1 << (n - 1)) | (1 << 4) | 1
    return n, hf, g, 5
