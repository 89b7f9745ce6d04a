"""What is read off the one- and two-particle density matrices of a state (``backend.Statevector.rdm1`` / ``rdm2``): natural orbitals
and their occupations, <N>, <S_z>, <S^2>, the energy re-assembled from integrals.  numpy only.

Conventions (``fermion.spin_orbital_integrals``): n spin orbitals, Jordan-Wigner, orbital p = qubit p, interleaved spins (even alpha,
odd beta);  gamma[p, q] = <a+_p a_q>,  Gamma[p, q, r, s] = <a+_p a+_q a_r a_s>,  packed D2[(p<q), (r<s)] = <a+_p a+_q a_s a_r> with the
pairs in lexicographic order."""
import numpy as np


def pair_index(n):
    """(P, 2) array of the pairs (p < q) in lexicographic order"""
    return np.array([(p, q) for p in range(n) for q in range(p + 1, n)], dtype=np.int64).reshape(-1, 2)


def unpack_rdm2(d2, n):
    """(P, P) D2 -> (n, n, n, n) Gamma by antisymmetry: Gamma[p,q,r,s] = -D2[(p,q),(r,s)] for p<q, r<s, the three permuted blocks
    by sign, zero where p = q or r = s"""
    d2 = np.asarray(d2)
    pr = pair_index(n)
    if d2.shape != (len(pr), len(pr)):
        raise ValueError(f"D2 of {n} orbitals is {len(pr)} x {len(pr)}, got {d2.shape}")
    g = np.zeros((n, n, n, n), d2.dtype)
    if len(pr) == 0:
        return g
    p, q = pr[:, 0][:, None], pr[:, 1][:, None]
    r, s = pr[:, 0][None, :], pr[:, 1][None, :]
    g[p, q, r, s] = -d2
    g[q, p, r, s] = d2
    g[p, q, s, r] = d2
    g[q, p, s, r] = -d2
    return g


def spin_summed_rdm1(g1):
    """D[i, j] = gamma[2i, 2j] + gamma[2i+1, 2j+1] over the spatial orbitals"""
    g1 = np.asarray(g1)
    return g1[0::2, 0::2] + g1[1::2, 1::2]


def natural_occupations(g1):
    """(NOONs descending, natural orbitals as columns) of the spin-summed one-particle density: the ``eigh`` and the reversal of
    ``chem.Molecule.natural_occupations``"""
    d = spin_summed_rdm1(g1)
    d = 0.5 * (d + d.conj().T)
    if np.abs(d.imag).max(initial=0.0) == 0.0:
        d = d.real
    w, v = np.linalg.eigh(d)
    return w[::-1].copy(), v[:, ::-1].copy()


def energy(hpq, hpqrs, constant, g1, g2):
    """constant + sum h_pq gamma_pq + 1/2 sum h_pqrs Gamma_pqrs (real part; g2: the (n,n,n,n) Gamma)"""
    e = np.einsum("pq,pq->", hpq, g1) + 0.5 * np.einsum("pqrs,pqrs->", hpqrs, g2)
    return float(constant + np.real(e))


def spin_expectations(g1, g2):
    """(<N>, <S_z>, <S^2>):  <n_p n_q> = delta_pq gamma_pp + Gamma[p,q,q,p],  S_z = 1/2 sum_i (n_2i - n_2i+1),
    S^2 = S_z + S_z^2 + sum_i gamma[2i+1, 2i+1] - sum_ij Gamma[2i+1, 2j, 2i, 2j+1]"""
    g1, g2 = np.asarray(g1), np.asarray(g2)
    n = g1.shape[0]
    occ = np.real(np.diagonal(g1))
    nn = np.real(np.einsum("pqqp->pq", g2)) + np.diag(occ)
    sgn = np.where(np.arange(n) % 2 == 0, 0.5, -0.5)
    sz = float(sgn @ occ)
    sz2 = float(sgn @ nn @ sgn)
    a, b = np.arange(0, n - 1, 2), np.arange(1, n, 2)
    s_minus_plus = float(occ[b].sum() - np.real(g2[b[:, None], a[None, :], a[:, None], b[None, :]]).sum())
    return float(occ.sum()), sz, sz + sz2 + s_minus_plus
