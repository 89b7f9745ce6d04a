"""Excited states by quantum subspace expansion (QSE; with an excitation pool the qEOM family) around the state in the buffer.

With expansion operators O_1 .. O_m and phi_j = O_j psi, the device forms S_ij = <phi_i|phi_j> and H_ij = <phi_i|H|phi_j>
(``Statevector.subspace_matrices``, ovqe_subspace_matrices); the generalised eigenproblem H y = E S y is solved here, on the host, by
canonical orthogonalisation.  The reference has no call site for this: its only excited-state code is a weighted subspace-search
demo on an Ising chain (ref:openvqe/common_files/get_energy_WSSVQE.py).

Excited states WITH ansatz parameters come from variational quantum deflation (``vqd``): state k minimises
C(theta) = <psi|H|psi> + sum_j beta_j |<phi_j|psi>|^2 over the states phi_j found before it; cost and exact gradient of a batch of
parameter vectors are one device call (``Statevector.deflated_gradient_batch``, ovqe_deflated_gradient_batch) and the optimiser is the
lock-step multi-start L-BFGS of ``common_files.multistart``.

A second route needs no stored vectors: the folded spectrum (``folded_spectrum``).  The minimum of S_omega = <psi|(H - omega)^2|psi>
over theta is the ansatz state nearest the chosen energy omega; S with its exact gradient for a batch is one device call
(``Statevector.spread_gradient_batch``, ovqe_spread_gradient_batch), and the energy variance of the result certifies it: an
eigenvalue of H lies within sqrt(variance) of its energy.
"""
from __future__ import annotations

import numpy as np

from . import fermion
from .operators import Hamiltonian


def excitation_operators(n_spatial, n_occ_spatial, deexcitations=False, identity=True):
    """The JW images of the BARE spin-conserving excitations a+_a a_i and a+_b a+_a a_i a_j of ``fermion.uccsd_excitations`` (not the
    anti-Hermitian generators): [identity,] singles, doubles [, their adjoints in the same order].  Complex coefficients."""
    nq = 2 * n_spatial
    singles, doubles = fermion.uccsd_excitations(n_spatial, n_occ_spatial)
    ladders = [([a], [i]) for i, a in singles] + [([b, a], [i, j]) for i, j, a, b in doubles]
    ops = [Hamiltonian(nq, [], 1.0)] if identity else []
    for creators, annihilators in ladders:
        t = fermion.jw_product([(p, True) for p in creators] + [(p, False) for p in annihilators])
        ops.append(fermion.psum_to_hamiltonian(nq, t, tol=1e-13))
    if deexcitations:
        for creators, annihilators in ladders:
            t = fermion.jw_product([(p, True) for p in reversed(annihilators)] + [(p, False) for p in reversed(creators)])
            ops.append(fermion.psum_to_hamiltonian(nq, t, tol=1e-13))
    return ops


def solve(H, S, rcond=1e-10):
    """H y = E S y by canonical orthogonalisation: eigenvectors of S with eigenvalue <= rcond * lambda_max are dropped, H is projected
    on the rest.  -> (energies ascending [rank], coefficients y [m, rank] with y^H S y = 1, rank)"""
    H = np.asarray(H, np.complex128)
    S = np.asarray(S, np.complex128)
    if H.shape != S.shape or H.ndim != 2 or H.shape[0] != H.shape[1]:
        raise ValueError("H and S must be square matrices of one size")
    w, U = np.linalg.eigh(0.5 * (S + S.conj().T))
    if w.size == 0 or w[-1] <= 0.0:
        raise ValueError("the overlap matrix has no positive eigenvalue: every expansion vector is zero")
    keep = w > rcond * w[-1]
    X = U[:, keep] / np.sqrt(w[keep])
    Hp = X.conj().T @ (0.5 * (H + H.conj().T)) @ X
    e, v = np.linalg.eigh(0.5 * (Hp + Hp.conj().T))
    return e, X @ v, int(keep.sum())


def qse(sv, ops, rcond=1e-10):
    """``sv.subspace_matrices(ops)`` followed by ``solve`` -> (energies, coefficients, rank)"""
    H, S = sv.subspace_matrices(ops)
    return solve(H, S, rcond)


def merged_pauli_sum(nbqbits, ops, y):
    """sum_j y_j O_j as one Pauli sum in index-space masks -> (xs, zs, coeffs); equal strings merged, constants on x = z = 0"""
    from .operators import pack_terms
    total = {}
    for yj, op in zip(np.asarray(y, np.complex128).reshape(-1), ops):
        xs, zs, cs = pack_terms(nbqbits, op.terms)
        for x, z, c in zip(xs.tolist(), zs.tolist(), cs.tolist()):
            total[(x, z)] = total.get((x, z), 0.0) + yj * c
        const = complex(getattr(op, "constant_coeff", 0.0) or 0.0)
        if const != 0:
            total[(0, 0)] = total.get((0, 0), 0.0) + yj * const
    keys = list(total)
    return (np.array([k[0] for k in keys], np.uint64), np.array([k[1] for k in keys], np.uint64),
            np.array([total[k] for k in keys], np.complex128))


def load_ritz_state(sv, ops, y):
    """puts the normalised sum_j y_j O_j psi into the state buffer of ``sv`` (psi: the state in the buffer): one merged Pauli sum
    through ``apply_pauli_sum``.  ``rdm1`` / ``rdm2`` / ``rdm.spin_expectations`` then describe the excited state.  -> the norm^2
    before normalisation (y^H S y: 1 for a column of ``solve``)"""
    y = np.asarray(y, np.complex128).reshape(-1)
    if y.shape[0] != len(ops):
        raise ValueError(f"expected {len(ops)} coefficients")
    xs, zs, cs = merged_pauli_sum(sv.nbqbits, ops, y)
    with type(sv)(sv.n_local, device=sv.device) as scratch:     # a second register of the same size: the sum cannot be applied in place
        buf = scratch.state_ptr()
        sv.apply_pauli_sum(xs, zs, cs, buf)
        state = sv.state_ptr()
        sv.vec_axpy(state, buf, 1.0, overwrite=True)
        norm2 = sv.norm2()          # (waits for the copy: the scratch register may go)
    if not norm2 > 0.0:
        raise ValueError("the Ritz vector is zero")
    sv.vec_scale(state, 1.0 / np.sqrt(norm2))
    return norm2


def spin_constraint(nbqbits, s=0.0, weight=None):
    """the constraint <S^2> = s (s + 1) for ``vqd(constraints=...)``: (``fermion.spin_squared(nbqbits)``, s (s + 1), ``weight``);
    ``weight=None``: 2 sum_t |c_t| of the stored Hamiltonian, the default of ``beta``"""
    return fermion.spin_squared(nbqbits), float(s) * (float(s) + 1.0), weight


def vqd(sv, n_states, x0=None, beta=None, starts=8, spread=0.5, seed=0, tol=1e-6, maxiter=2000, constraints=None):
    """Variational quantum deflation on the program and Hamiltonian loaded in ``sv``: for k = 0 .. n_states - 1 the cost
    C = <H> + sum_j beta_j |<phi_j|psi(theta)>|^2 over the deflation vectors ``sv`` holds is minimised from ``starts`` starting vectors in
    lock-step (``multistart.minimize``, one ``deflated_gradient_batch`` call per iteration) — start 0 is ``x0`` (zeros by default), the
    others are ``x0`` plus uniform draws from [-spread, spread], as ``EnergyUCC.multistart`` draws them — then the best start's state is
    prepared and pushed with weight ``beta``.  ``beta=None``: 2 sum_t |c_t| of the stored Hamiltonian without its constant — more than
    its spectral width, so every deflated level lies above every level not yet found.  Vectors pushed before the call (a Lanczos ground
    state, say) are built upon; when the call leaves, normally or not, the set is truncated back to what it found.
    ``constraints``: a list of (operator, target, quad_weight) — ``spin_constraint`` builds one — adds quad_weight (<operator> - target)^2
    to every state's cost: the operators are pushed behind the observables ``sv`` holds (those enter with weight zero), every iteration
    is one ``constrained_gradient_batch`` call, and the observables are truncated back when the call leaves.  A weight of None is
    2 sum_t |c_t| of the stored Hamiltonian.  With ``constraints=None`` the observables are not touched.
    -> a list of ``n_states`` dicts: ``energy``, ``cost``, ``theta``, ``overlaps`` (complex, with the vectors held before state k was
    pushed: the earlier states last) and ``result`` (the multistart result); with constraints also ``values``, the expectation values
    of the observables held"""
    from .common_files import multistart
    K = sv._K
    x0 = np.zeros(K) if x0 is None else np.asarray(x0, np.float64).reshape(-1)
    if x0.shape[0] != K:
        raise ValueError(f"expected {K} parameters")
    if int(starts) < 1:
        raise ValueError("starts: at least one")
    beta = 2.0 * sv.hamiltonian_norm1() if beta is None else float(beta)
    rng = np.random.default_rng(seed)
    found = sv.deflation_count()
    states = []
    if constraints is not None:
        return _vqd_constrained(sv, int(n_states), x0, beta, int(starts), spread, rng, tol, maxiter, list(constraints), found)
    try:
        for _ in range(int(n_states)):
            X0 = np.tile(x0, (int(starts), 1))
            X0[1:] += rng.uniform(-spread, spread, size=(int(starts) - 1, K))
            res = multistart.minimize(lambda X: sv.deflated_gradient_batch(X)[:2], X0, tol=tol, maxiter=maxiter)
            cost, _, energy, overlaps = sv.deflated_gradient_batch(res.x[None, :])
            states.append({"energy": float(energy[0]), "cost": float(cost[0]), "theta": res.x.copy(), "overlaps": overlaps[0].copy(),
                           "result": res})
            sv.prepare_state(res.x)
            sv.deflation_push(beta)
    finally:
        sv.deflation_truncate(found)
    return states


def _vqd_constrained(sv, n_states, x0, beta, starts, spread, rng, tol, maxiter, constraints, found):
    """``vqd`` with penalty terms: the same loop on ``constrained_gradient_batch``"""
    from .common_files import multistart
    K = sv._K
    held = sv.observable_count()
    quad = np.zeros(held + len(constraints))
    target = np.zeros(held + len(constraints))
    states = []
    try:
        for m, (operator, want, weight) in enumerate(constraints):
            sv.observable_push(operator)
            target[held + m] = float(want)
            quad[held + m] = 2.0 * sv.hamiltonian_norm1() if weight is None else float(weight)
        for _ in range(n_states):
            X0 = np.tile(x0, (starts, 1))
            X0[1:] += rng.uniform(-spread, spread, size=(starts - 1, K))
            res = multistart.minimize(lambda X: sv.constrained_gradient_batch(X, quad=quad, target=target)[:2], X0, tol=tol, maxiter=maxiter)
            cost, _, energy, values, overlaps = sv.constrained_gradient_batch(res.x[None, :], quad=quad, target=target)
            states.append({"energy": float(energy[0]), "cost": float(cost[0]), "theta": res.x.copy(), "overlaps": overlaps[0].copy(),
                           "values": values[0].copy(), "result": res})
            sv.prepare_state(res.x)
            sv.deflation_push(beta)
    finally:
        sv.deflation_truncate(found)
        sv.observable_truncate(held)
    return states


def folded_spectrum(sv, omegas, x0=None, starts=8, spread=0.5, seed=0, tol=1e-6, maxiter=2000):
    """Folded-spectrum states on the program and Hamiltonian loaded in ``sv``: for every omega in ``omegas`` the cost
    S = <psi(theta)|(H - omega)^2|psi(theta)> is minimised from ``starts`` starting vectors in lock-step (``multistart.minimize``, one
    ``spread_gradient_batch`` call per iteration) — start 0 is ``x0`` (zeros by default), the others are ``x0`` plus uniform draws from
    [-spread, spread], as ``vqd`` draws them.  The best start is then evaluated once in variance mode.
    -> a list with one dict per omega: ``theta``, ``energy`` = <H>, ``spread`` = S at the minimum, ``variance`` = <H^2> - <H>^2 there, and
    ``result`` (the multistart result).  The variance is the certificate: an eigenvalue of H lies within sqrt(variance) of ``energy``
    (spread = variance + (energy - omega)^2)."""
    from .common_files import multistart
    K = sv._K
    x0 = np.zeros(K) if x0 is None else np.asarray(x0, np.float64).reshape(-1)
    if x0.shape[0] != K:
        raise ValueError(f"expected {K} parameters")
    if int(starts) < 1:
        raise ValueError("starts: at least one")
    rng = np.random.default_rng(seed)
    states = []
    for omega in np.asarray(omegas, np.float64).reshape(-1):
        X0 = np.tile(x0, (int(starts), 1))
        X0[1:] += rng.uniform(-spread, spread, size=(int(starts) - 1, K))
        res = multistart.minimize(lambda X: sv.spread_gradient_batch(X, omega=float(omega))[:2], X0, tol=tol, maxiter=maxiter)
        _, _, energy, variance = sv.spread_gradient_batch(res.x[None, :])
        states.append({"theta": res.x.copy(), "energy": float(energy[0]), "spread": float(res.fun), "variance": float(variance[0]),
                       "result": res})
    return states
