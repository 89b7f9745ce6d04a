"""TEST INFRASTRUCTURE ONLY — observables beside the Hamiltonian (ovqe_constrained_gradient_batch) and spin-pure VQD
(openvqe_amd/excited.py: vqd(constraints=...)): the checker, the bounds, the stand-in backend and the small observable builders of
tests/test_constraint_cases.py / tests/test_gpu_constraints.py.

The checker is ``deflation_cases.deflated_gradient`` restated with lambda += sum_m g_m O_m psi, g_m = linear_m + 2 quad_m (o_m - target_m),
on the dense complex register — no finite differences.  Literal gate lists: the same lambda against the forward tangents of
``metric_cases.gate_tangents``.  An observable is a tuple (xs, zs, coeffs, constant) in index-space masks (``pack``)."""
import numpy as np

from oracle import masks
from tests import deflation_cases as dc
from tests import gradbatch_cases as gc
from tests import metric_cases


def pack(n, operator):
    """a ``Hamiltonian`` -> (xs, zs, real coeffs, real constant)"""
    from openvqe_amd.operators import pack_terms
    xs, zs, cs = pack_terms(n, operator.terms)
    assert np.abs(np.imag(cs)).max(initial=0.0) < 1e-12
    return xs, zs, np.real(cs).astype(np.float64), float(np.real(operator.constant_coeff or 0.0))


def norm1(obs):
    """||O||_1 = sum_t |c_t| + |constant|"""
    return float(np.abs(obs[2]).sum()) + abs(float(obs[3]))


def _weights(M, linear, quad, target):
    z = np.zeros(M)
    return [z if w is None else np.asarray(w, np.float64).reshape(M) for w in (linear, quad, target)]


# ---- the checker --------------------------------------------------------------------------------------------------------------------------
def _observables(psi, lam, observables, linear, quad, target):
    """(values o_m, sum_m [linear_m o_m + quad_m (o_m - target_m)^2], lambda + sum_m g_m O_m psi)"""
    lin, qd, tg = _weights(len(observables), linear, quad, target)
    values, pen = np.zeros(len(observables)), 0.0
    for m, (xs, zs, cs, const) in enumerate(observables):
        sigma = masks.apply_pauli_sum(psi, xs, zs, cs)
        o = float(np.vdot(psi, sigma).real) + const
        values[m] = o
        pen += lin[m] * o + qd[m] * (o - tg[m]) ** 2
        lam = lam + (lin[m] + 2.0 * qd[m] * (o - tg[m])) * sigma
    return values, pen, lam


def constrained_gradient(n, hf, rx, rz, rc, pidx, theta, hx, hz, hc, constant=0.0, phi0=None, observables=(), linear=None, quad=None,
                         target=None, vectors=(), betas=()):
    """-> (C, dC/dtheta[K], E, o[M], overlaps[J]) of the rotation program"""
    phis = masks._angles(rc, pidx, theta, phi0)
    psi = masks.ucc_state(n, hf, rx, rz, rc, pidx, theta, phi0)
    lam = masks.apply_pauli_sum(psi, hx, hz, hc)
    energy = float(np.vdot(psi, lam).real) + float(np.real(constant))
    o, pen, lam = dc._penalty(psi, lam, vectors, betas)
    values, pen_o, lam = _observables(psi, lam, observables, linear, quad, target)
    grad = np.zeros(len(theta), np.float64)
    for r in range(len(rc) - 1, -1, -1):
        x, z = int(rx[r]), int(rz[r])
        if int(pidx[r]) >= 0:
            grad[int(pidx[r])] += 2.0 * float(rc[r]) * float(np.vdot(lam, masks.pauli_apply(psi, x, z)).imag)
        psi = masks.rotate(psi, x, z, -phis[r])
        lam = masks.rotate(lam, x, z, -phis[r])
    return energy + pen + pen_o, grad, energy, values, o


def constrained_gradient_gates(n, hf, gates, theta, hx, hz, hc, constant=0.0, observables=(), linear=None, quad=None, target=None,
                               vectors=(), betas=()):
    """the same for a literal gate list"""
    psi, T = metric_cases.gate_tangents(n, hf, gates, theta)
    lam = masks.apply_pauli_sum(psi, hx, hz, hc)
    energy = float(np.vdot(psi, lam).real) + float(np.real(constant))
    o, pen, lam = dc._penalty(psi, lam, vectors, betas)
    values, pen_o, lam = _observables(psi, lam, observables, linear, quad, target)
    grad = np.array([2.0 * float(np.vdot(T[k], lam).real) for k in range(len(theta))], np.float64).reshape(len(theta))
    return energy + pen + pen_o, grad, energy, values, o


def case_want(case, theta, observables=(), linear=None, quad=None, target=None, vectors=(), betas=()):
    """the checker on a ``gradbatch_cases.Case``"""
    return constrained_gradient(case.n, case.hf, case.rx, case.rz, case.rc, case.pidx, np.ascontiguousarray(theta, np.float64), *case.h,
                                case.phi0, observables, linear, quad, target, vectors, betas)


# ---- bounds -------------------------------------------------------------------------------------------------------------------------------
def weight(h1, observables=(), linear=None, quad=None, target=None, vectors=(), betas=()):
    """W = the deflation weight + sum_m (|linear_m| + 2 |quad_m| (||O_m||_1 + |target_m|)) ||O_m||_1: the worst-case 1-norm of the
    effective operator H + sum_j beta_j |phi_j><phi_j| + sum_m g_m O_m, |g_m| <= |linear_m| + 2 |quad_m| (||O_m||_1 + |target_m|)"""
    lin, qd, tg = _weights(len(observables), linear, quad, target)
    w = dc.weight(h1, vectors, betas)
    for m, obs in enumerate(observables):
        w += (abs(lin[m]) + 2.0 * abs(qd[m]) * (norm1(obs) + abs(tg[m]))) * norm1(obs)
    return w


def bound_checker(h1, C, *args, **kwargs):
    return gc.bound_checker(weight(h1, *args, **kwargs), C)


def bound_single(h1, C, *args, **kwargs):
    """against another call on the same handle"""
    return gc.bound_single(weight(h1, *args, **kwargs), C)


def bound_value(obs, other_call=False):
    """a value o_bm: 1e-10 ||O_m||_1 against the checker, 1e-12 ||O_m||_1 against another call"""
    return (1e-12 if other_call else 1e-10) * max(norm1(obs), 1e-300)


# ---- small observables --------------------------------------------------------------------------------------------------------------------
def from_masks(n, xs, zs, cs, constant=0.0):
    """index-space masks -> a ``Hamiltonian`` (``hessian_cases.hamiltonian_object``)"""
    from tests import hessian_cases
    return hessian_cases.hamiltonian_object(n, np.asarray(xs, np.uint64), np.asarray(zs, np.uint64), np.asarray(cs, np.float64), constant)


def random_observable(n, nterms, seed, x_pool=None, constant=0.0):
    """a random real Pauli sum whose x masks come from ``x_pool`` (the program's, so that it couples support states) and 0"""
    from tests import hessian_cases
    hx, hz, hc = hessian_cases.random_real_hamiltonian(n, nterms, seed, x_pool=x_pool)
    return hessian_cases.hamiltonian_object(n, hx, hz, hc, constant)


def diagonal_observable(n, seed, constant=0.0):
    """sum_q c_q Z_q"""
    rng = np.random.default_rng(seed)
    return from_masks(n, [0] * n, [1 << q for q in range(n)], rng.uniform(-1.0, 1.0, n), constant)


def odd_y_only(n, constant=0.5):
    """Y_0 + 0.5 Y_1 X_2 (where n allows): every term has an odd number of Y — no restricted entry on any support"""
    xs, zs, cs = [1], [1], [1.0]
    if n >= 3:
        xs.append(0b110)
        zs.append(0b010)
        cs.append(0.5)
    return from_masks(n, xs, zs, cs, constant)


# ---- the stand-in backend ---------------------------------------------------------------------------------------------------------------
class ConstraintOracle(dc.DeflationOracle):
    """the CPU stand-in with the observable surface of ``Statevector``, from the checker (rotation programs)"""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._observables = []

    def observable_push(self, hamiltonian):
        if len(self._observables) >= 8:
            raise ValueError("count")
        self._observables.append(pack(self.nbqbits, hamiltonian))
        return len(self._observables)

    def observable_truncate(self, count=0):
        if not 0 <= count <= len(self._observables):
            raise ValueError("count")
        del self._observables[count:]

    def observable_count(self):
        return len(self._observables)

    def constrained_gradient_batch(self, thetas, linear=None, quad=None, target=None):
        thetas = np.ascontiguousarray(thetas, np.float64)
        if thetas.ndim != 2 or thetas.shape[1] != self._K:
            raise ValueError("shape")
        _, xs, zs, cs, p0, pi, hf = self._prog
        hx, hz, hc, const = self._ham
        out = [constrained_gradient(self.nbqbits, hf, xs, zs, cs, pi, t, hx, hz, hc, const, p0, self._observables, linear, quad, target,
                                    self._vectors, self._betas) for t in thetas]
        B, M, J = len(out), len(self._observables), len(self._vectors)
        self._info = dict(path=2, B=B, K=self._K, M=M, J=J)
        return (np.array([r[0] for r in out]), np.array([r[1] for r in out]).reshape(B, thetas.shape[1]), np.array([r[2] for r in out]),
                np.array([r[3] for r in out]).reshape(B, M), np.array([r[4] for r in out], np.complex128).reshape(B, J))

    def expectations_batch(self, thetas):
        _, _, e, v, _ = self.constrained_gradient_batch(thetas)
        return e, v

    def constraint_info(self):
        return dict(self._info)
