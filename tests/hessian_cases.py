"""TEST INFRASTRUCTURE ONLY — exact checkers of the energy Hessian (ovqe_energy_hessian) on the dense register, the case helpers of
tests/test_hessian_cases.py / tests/test_gpu_hessian.py, and the restatement of the compact kernel's LDS formula.

``rotation_hessian`` / ``gate_hessian`` are forward over forward: psi, the first tangents T_k = d psi / d theta_k and the second
tangents T_bk = d2 psi / d theta_b d theta_k go through the program by nested forward mode (``metric_cases.rotation_tangents`` /
``gate_tangents`` one order up, Pauli strings applied with the index and sign arithmetic of ``oracle.masks.pauli_apply``), and

    H_bk = 2 Re <T_b|H|T_k> + 2 Re <psi|H|T_bk>:

no finite differences.  Behind a rotation exp(-i phi P), phi = c theta_p + c0, with a prime for the rotated vectors:
    T_bk <- T_bk' + [k = p] c (-i P) T_b' + [b = p] c (-i P) T_k' + [b = k = p] c^2 (-i P)^2 psi',    T_p <- T_p' + c (-i P) psi'.
That costs K^2 vectors per rotation.  ``rotation_hessian_adjoint`` is the O(K) form on the same dense complex register — the adjoint
pass of ``oracle.masks.ucc_energy_gradient`` differentiated in every direction — for the cases whose K^2 2^n second tangents do not
fit a test (LiH: 92^2 x 4096); tests/test_hessian_cases.py holds it to the nested form where both run.  ``hessian`` picks between them."""
import numpy as np

from oracle import dense, masks
from tests import metric_cases

NESTED_LIMIT = 1 << 22   # K^2 2^n second-tangent amplitudes (64 MiB) up to which ``hessian`` runs the nested forward mode


def _index_sign(n_amps, x, z):
    """j = i ^ x and (-1)^{parity((i ^ x) & z)} of ``masks.pauli_apply``"""
    idx = np.arange(n_amps, dtype=np.uint64)
    j = np.arange(n_amps, dtype=np.int64) ^ int(x)
    return j, 1.0 - 2.0 * masks._parity((idx ^ np.uint64(x)) & np.uint64(z))


def _scaled(A, f, j):
    return f.reshape((A.shape[0],) + (1,) * (A.ndim - 1)) * A[j]


def _pauli_cols(A, x, z):
    """P applied to every column of the (2^n, ...) array A: ``masks.pauli_apply`` on axis 0.  An even number of Y: a real matrix"""
    j, sign = _index_sign(A.shape[0], x, z)
    ny = masks._popcount_int(int(x) & int(z)) % 4
    return _scaled(A, ((1j) ** ny * sign) if ny & 1 else ((-1.0 if ny == 2 else 1.0) * sign), j)


def _q_cols(A, x, z):
    """Q = -i P on every column.  An odd number of Y: a real matrix (the rotations of a real program keep float64 arrays real)"""
    j, sign = _index_sign(A.shape[0], x, z)
    ny = masks._popcount_int(int(x) & int(z)) % 4
    return _scaled(A, ((1.0 if ny == 1 else -1.0) * sign) if ny & 1 else (-1j * (1j) ** ny * sign), j)


def _rotate_cols(A, x, z, phi):
    """exp(-i phi P) = cos(phi) + sin(phi) Q"""
    return np.cos(phi) * A + np.sin(phi) * _q_cols(A, x, z)


def _dtype(rx, rz, hx, hz):
    """float64 when every rotation string has an odd and every Hamiltonian string an even number of Y (nothing leaves the reals)"""
    odd = all(masks._popcount_int(int(x) & int(z)) & 1 for x, z in zip(rx, rz))
    even = all(not masks._popcount_int(int(x) & int(z)) & 1 for x, z in zip(hx, hz))
    return np.float64 if odd and even else np.complex128


def _h_cols(A, hx, hz, hc):
    """H on every column, one gather per x mask"""
    groups = {}
    for x, z, c in zip(hx, hz, hc):
        j, sign = _index_sign(A.shape[0], int(x), int(z))
        ny = masks._popcount_int(int(x) & int(z)) % 4
        f = complex(c) * (1j) ** ny * sign
        groups[int(x)] = (j, groups[int(x)][1] + f) if int(x) in groups else (j, f)
    out = np.zeros_like(A)
    for j, f in groups.values():
        out += _scaled(A, f if np.iscomplexobj(A) else f.real, j)
    return out


def _finish(psi, T, S, hx, hz, hc, constant):
    """(E, grad, hess) from psi (N), T (N, K), S (N, K, K)"""
    lam = _h_cols(psi, hx, hz, hc)
    HT = _h_cols(T, hx, hz, hc)
    e = float(np.vdot(psi, lam).real) + float(np.real(constant))
    grad = 2.0 * (lam.conj() @ T).real
    hess = 2.0 * (T.conj().T @ HT).real + 2.0 * np.tensordot(lam.conj(), S, axes=(0, 0)).real
    return e, grad, 0.5 * (hess + hess.T)


def _inject(psi, T, S, x, z, c, p):
    """the three vectors behind a rotated step whose angle is c theta_p + ...; c Q = c (-i P) applied to the ROTATED vectors"""
    QT = c * _q_cols(T, x, z)
    Qpsi = c * _q_cols(psi, x, z)
    S[:, p, :] += QT
    S[:, :, p] += QT
    S[:, p, p] += c * _q_cols(Qpsi, x, z)
    T[:, p] += Qpsi


def rotation_hessian(n, hf, rx, rz, rc, pidx, theta, hx, hz, hc, constant=0.0, phi0=None):
    """nested forward mode -> (E, grad[K], hess[K, K]) of prod_r exp(-i (rc_r theta[pidx_r] + phi0_r) P_r)|hf>, rotation 0 first"""
    K, N, dt = len(theta), 1 << n, _dtype(rx, rz, hx, hz)
    psi = np.zeros(N, dt)
    psi[int(hf)] = 1.0
    T = np.zeros((N, K), dt)
    S = np.zeros((N, K, K), dt)
    phi0 = np.zeros(len(rx)) if phi0 is None else phi0
    for x, z, c, c0, p in zip(rx, rz, rc, phi0, pidx):
        x, z, p, c = int(x), int(z), int(p), float(c)
        phi = metric_cases._angle(c, c0, p, theta)
        psi, T, S = _rotate_cols(psi, x, z, phi), _rotate_cols(T, x, z, phi), _rotate_cols(S, x, z, phi)
        if p >= 0:
            _inject(psi, T, S, x, z, c, p)
    return _finish(psi, T, S, hx, hz, hc, constant)


def gate_hessian(n, hf, gates, theta, hx, hz, hc, constant=0.0):
    """nested forward mode of a literal gate list [(name, qubits, angle_scale, angle_const, param or -1)] (``metric_cases.gate_tangents``)"""
    K, N = len(theta), 1 << n
    psi = np.zeros(N, np.complex128)
    psi[int(hf)] = 1.0
    T = np.zeros((N, K), np.complex128)
    S = np.zeros((N, K, K), np.complex128)

    def cols(fn, A):
        flat = A.reshape(N, -1)
        return np.stack([fn(flat[:, q]) for q in range(flat.shape[1])], axis=1).reshape(A.shape) if flat.shape[1] else A

    for name, qubits, scale, const, p in gates:
        if name in metric_cases._AXIS:
            x, z = masks.pack_pauli(n, metric_cases._AXIS[name], [qubits[0]])
            phi = 0.5 * metric_cases._angle(scale, const, p, theta)
            psi, T, S = _rotate_cols(psi, x, z, phi), _rotate_cols(T, x, z, phi), _rotate_cols(S, x, z, phi)
            if p >= 0:
                _inject(psi, T, S, x, z, 0.5 * float(scale), p)
        elif name == "CNOT":
            fn = lambda v: masks.gate_cnot(v, n, qubits[0], qubits[1])   # noqa: E731
            psi, T, S = fn(psi), cols(fn, T), cols(fn, S)
        else:
            m = dense.gate_matrix(name, 0.0)
            fn = lambda v: masks.gate_1q(v, n, qubits[0], m)   # noqa: E731
            psi, T, S = fn(psi), cols(fn, T), cols(fn, S)
    return _finish(psi, T, S, hx, hz, hc, constant)


def rotation_hessian_adjoint(n, hf, rx, rz, rc, pidx, theta, hx, hz, hc, constant=0.0, phi0=None):
    """the O(K) form: first tangents forward, lambda = H psi and mu_b = H T_b, then the rotations backwards on all of them.  With
    Q = -i P, Im <a|P|b> = Re <a|Q b>:  w'_r[b] = 2 Re(<mu_b|Q_r psi> + <lambda|Q_r T_b>) before rotation r is un-applied, then
    T_p -= c Q psi and mu_p -= c Q lambda (= + c (i P) ...) of the un-applied vectors -> (E, grad, hess, max |M - M^T| of the raw rows)"""
    K, N, R, dt = len(theta), 1 << n, len(rx), _dtype(rx, rz, hx, hz)
    psi = np.zeros(N, dt)
    psi[int(hf)] = 1.0
    T = np.zeros((N, K), dt)
    phi0 = np.zeros(R) if phi0 is None else phi0
    phis = [metric_cases._angle(rc[r], phi0[r], int(pidx[r]), theta) for r in range(R)]
    for r in range(R):
        x, z, p = int(rx[r]), int(rz[r]), int(pidx[r])
        psi, T = _rotate_cols(psi, x, z, phis[r]), _rotate_cols(T, x, z, phis[r])
        if p >= 0:
            T[:, p] += float(rc[r]) * _q_cols(psi, x, z)
    lam, MU = _h_cols(psi, hx, hz, hc), _h_cols(T, hx, hz, hc)
    e = float(np.vdot(psi, lam).real) + float(np.real(constant))
    grad, M = np.zeros(K), np.zeros((K, K))
    for r in range(R - 1, -1, -1):
        x, z, p, c = int(rx[r]), int(rz[r]), int(pidx[r]), float(rc[r])
        cs, sn = np.cos(phis[r]), np.sin(phis[r])
        Qpsi, Qlam, QT, QMU = _q_cols(psi, x, z), _q_cols(lam, x, z), _q_cols(T, x, z), _q_cols(MU, x, z)
        if p >= 0:
            grad[p] += 2.0 * c * float(np.vdot(lam, Qpsi).real)
            M[:, p] += 2.0 * c * ((MU.conj().T @ Qpsi).real + (lam.conj() @ QT).real)
        psi, lam, T, MU = cs * psi - sn * Qpsi, cs * lam - sn * Qlam, cs * T - sn * QT, cs * MU - sn * QMU   # exp(+i phi P)
        if p >= 0:
            T[:, p] -= c * _q_cols(psi, x, z)
            MU[:, p] -= c * _q_cols(lam, x, z)
    return e, grad, 0.5 * (M + M.T), float(np.abs(M - M.T).max()) if K else 0.0


def hessian(n, hf, rx, rz, rc, pidx, theta, hx, hz, hc, constant=0.0, phi0=None):
    """(E, grad, hess) by the nested forward mode where its K^2 2^n second tangents fit NESTED_LIMIT, else by the adjoint form"""
    if len(theta) ** 2 << n <= NESTED_LIMIT:
        return rotation_hessian(n, hf, rx, rz, rc, pidx, theta, hx, hz, hc, constant, phi0)
    return rotation_hessian_adjoint(n, hf, rx, rz, rc, pidx, theta, hx, hz, hc, constant, phi0)[:3]


# ---- bounds and the checks every GPU result gets ------------------------------------------------------------------------------------
def norm1(hc, constant=0.0):
    return float(np.abs(np.asarray(hc, np.complex128)).sum()) + abs(float(np.real(constant)))


def coefficient_sum(rc, pidx, K):
    """C = max_k sum_{r in k} |coeff_r|"""
    tot = np.zeros(max(K, 1))
    for c, p in zip(rc, pidx):
        if int(p) >= 0:
            tot[int(p)] += abs(float(c))
    return float(tot.max())


def bound(h1, C):
    """|delta H_bk| <= 1e-10 ||H||_1 max(1, C^2): the project's 1e-10 ||H||_1 energy bound carried through two derivatives"""
    return 1e-10 * h1 * max(1.0, C * C)


def call_hessian(sv, theta, path, h1, C):
    """energy_hessian with the checks every result gets -> (e, grad, hess, info)"""
    e, grad, hess = sv.energy_hessian(theta)
    info = sv.hessian_info()
    K = len(theta)
    assert hess.shape == (K, K) and hess.dtype == np.float64 and grad.shape == (K,)
    assert np.array_equal(hess.view(np.int64), hess.T.copy().view(np.int64))
    assert info["path"] == path and info["K"] == K, info
    print(f"path {path} K {K} asymmetry {info['asymmetry']:.3e} bound {bound(h1, C):.3e} info {info}")
    assert 0.0 <= info["asymmetry"] <= bound(h1, C)
    e2, g2 = sv.energy_gradient(theta)
    print(f"   |e - e_grad| {abs(e - e2):.3e}  max|grad - grad_grad| {np.abs(grad - g2).max() if K else 0.0:.3e}  bound {1e-12 * h1:.3e}")
    assert abs(e - e2) <= 1e-12 * h1 and (K == 0 or np.abs(grad - g2).max() <= 1e-12 * h1)
    return e, grad, hess, info


def compare(hess, want, what, h1, C):
    err = float(np.abs(hess - want).max()) if hess.size else 0.0
    print(f"{what}: max|delta H| = {err:.3e}, bound {bound(h1, C):.3e}, max|H| = {np.abs(want).max() if want.size else 0:.4f}")
    assert err <= bound(h1, C)


def random_real_hamiltonian(n, nterms, seed, identity=True, x_pool=None):
    """random strings with an even number of Y (a real-symmetric sum), an identity term and a Z-only term first -> (hx, hz, hc).
    ``x_pool``: the x masks are 0, a member of the pool or the XOR of two (the rotation masks of a program: terms that connect the
    states of its support, which random masks on a wide register hardly ever do)"""
    rng = np.random.default_rng(seed)
    xs, zs = [0, 0], [0, int(rng.integers(1, 1 << n))]
    pool = None if x_pool is None else sorted({int(x) for x in x_pool})
    tries = 0
    while len(xs) < nterms and tries < 100 * nterms:
        tries += 1
        if pool is None:
            x = int(rng.integers(0, 1 << n))
        else:
            x = [0, pool[int(rng.integers(len(pool)))], pool[int(rng.integers(len(pool)))] ^ pool[int(rng.integers(len(pool)))]][int(rng.integers(3))]
        z = int(rng.integers(0, 1 << n))
        if bin(x & z).count("1") % 2 == 0 and (x, z) not in zip(xs, zs):
            xs.append(x)
            zs.append(z)
    hc = rng.uniform(-1.0, 1.0, len(xs))
    if not identity:
        xs, zs, hc = xs[1:], zs[1:], hc[1:]
    return np.array(xs, np.uint64), np.array(zs, np.uint64), hc


def hamiltonian_object(n, hx, hz, hc, constant=0.0):
    """``openvqe_amd.operators.Hamiltonian`` of packed strings (bit n - 1 - q = qubit q, as ``masks.pack_pauli``)"""
    from openvqe_amd.operators import Hamiltonian, Term
    terms = []
    for x, z, c in zip(hx, hz, hc):
        ops, qubits = "", []
        for q in range(n):
            bx, bz = (int(x) >> (n - 1 - q)) & 1, (int(z) >> (n - 1 - q)) & 1
            if bx or bz:
                ops += "Y" if bx and bz else "X" if bx else "Z"
                qubits.append(q)
        terms.append(Term(float(c), ops, qubits))
    return Hamiltonian(n, terms, float(constant))


# ---- the compact kernel's LDS (sp_hessian_lds, csrc/sv_sparse.hpp) -------------------------------------------------------------------
LDS_WG_BUDGET = 150 * 1024


def hessian_lds_bytes(m, ntab, K, nops, npairs, stage):
    """psi, the tangent, lambda and mu ([mpad] doubles each), cos / sin (16 bytes) and dk, w, wd (8 bytes each) per table entry, gk [K],
    rounded up to 16 bytes; staged: the 16-byte op records and the 4-byte pair words behind them"""
    mpad = (m + 1) & ~1
    base = (4 * mpad * 8 + ntab * 40 + K * 8 + 15) & ~15
    return base + nops * 16 + npairs * 4 if stage else base


def hessian_form(m, ntab, K, nops, npairs):
    """(form, LDS bytes) the way run_hessian chooses: 1 staged, 2 unstaged, 0 streaming although a compact program exists"""
    staged, plain = hessian_lds_bytes(m, ntab, K, nops, npairs, True), hessian_lds_bytes(m, ntab, K, nops, npairs, False)
    if staged <= LDS_WG_BUDGET:
        return 1, staged
    return (2, plain) if plain <= LDS_WG_BUDGET else (0, 0)


def streaming_workspace(n, K, records):
    """hessian::streaming_layout (csrc/sv_hessian_host.hpp): two stores of 2^n rows x wpad 16-byte amplitudes (K + 1 columns padded to
    64), the slab sums of one weight reduction (at most 256 slabs of at least four rows, wpad doubles each) and ``records`` weight
    records of wpad doubles — the energy and one per parameterised rotation with a coefficient"""
    rows, wpad = 1 << n, (K + 1 + 63) // 64 * 64
    slab_rows = max(4, (rows + 255) // 256)
    nslabs = (rows + slab_rows - 1) // slab_rows
    return 2 * rows * wpad * 16 + nslabs * wpad * 8 + records * wpad * 8


def cube_boundaries(n, K):
    """R of the last staged, first unstaged, last unstaged and first streaming ``metric_cases.cube_program(n, R, K, seed)``"""
    form = lambda R: hessian_form(*_cube(n, R, K))[0]   # noqa: E731
    R = n
    assert form(R) == 1
    while form(R + 1) == 1:
        R += 1
    last_staged = R
    assert form(R + 1) == 2
    R += 1
    while form(R + 1) == 2:
        R += 1
    return last_staged, last_staged + 1, R, R + 1


def _cube(n, R, K):
    m, ntab, nops, npairs = metric_cases.cube_sizes(n, R)
    return m, ntab, K, nops, npairs
