"""TEST INFRASTRUCTURE ONLY — exact forward-mode checker of the Fubini-Study metric (ovqe_metric_tensor) and the case lists of
tests/test_metric_cases.py / tests/test_gpu_metric.py.

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
