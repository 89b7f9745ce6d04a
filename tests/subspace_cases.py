"""TEST INFRASTRUCTURE ONLY — checker of the subspace-expansion matrices (ovqe_subspace_matrices) and the case builders of
tests/test_subspace_cases.py / tests/test_gpu_subspace.py, with the tolerance every GPU result is held to.

The checker builds Phi (phi_j = O_j psi) and Sigma (sigma_j = H phi_j, constant included) in numpy with
``oracle.masks.apply_pauli_sum`` — from n = 10 on H is built ONCE as a scipy.sparse matrix from the packed terms — and returns
S = Phi^H Phi, G = Phi^H Sigma and the expected row count, the definition of R evaluated literally:
R = { i : psi[i ^ x] != 0 for some distinct x mask of the pool }.

TOLERANCE, from the project's own bars (amplitudes 1e-12, energies 1e-10 ||H||_1): with a_j = sum_t |c_t| of operator j and psi
normalised,  |S_ij - want| <= 1e-12 a_i a_j,   |G_ij - want| <= 1e-10 (||H||_1 + |constant|) a_i a_j,  real and imaginary parts both
(which side is conjugated is part of the contract)."""
import numpy as np

from openvqe_amd import fermion
from openvqe_amd.operators import Hamiltonian, Term, pack_terms
from oracle import masks
from tests import util


def packed_ops(n, ops):
    """[(xs, zs, coeffs)] per operator in index-space masks, the constant as a term on the identity string"""
    out = []
    for op in ops:
        xs, zs, cs = pack_terms(n, op.terms)
        xs, zs, cs = [int(x) for x in xs], [int(z) for z in zs], [complex(c) for c in cs]
        const = complex(getattr(op, "constant_coeff", 0.0) or 0.0)
        if const != 0:
            xs, zs, cs = xs + [0], zs + [0], cs + [const]
        out.append((xs, zs, cs))
    return out


def weights(n, ops):
    """a_j = sum_t |c_t|"""
    return np.array([sum(abs(c) for c in cs) for _, _, cs in packed_ops(n, ops)])


def h_norm1(ham):
    return float(sum(abs(complex(t.coeff)) for t in ham.terms)) + abs(complex(ham.constant_coeff))


def expected_rows(psi, n, ops):
    xs = sorted({x for pxs, _, _ in packed_ops(n, ops) for x in pxs})
    nz = psi != 0
    idx = np.arange(1 << n)
    hit = np.zeros(1 << n, bool)
    for x in xs:
        hit |= nz[idx ^ x]
    return int(hit.sum())


def phi_sigma(psi, n, ops, ham):
    """(Phi [m, 2^n], Sigma [m, 2^n] or None without a Hamiltonian)"""
    Phi = np.array([masks.apply_pauli_sum(psi, xs, zs, cs) if xs else np.zeros_like(psi) for xs, zs, cs in packed_ops(n, ops)])
    if ham is None:
        return Phi, None
    if n >= 10:
        Sigma = (ham.get_matrix(sparse=True) @ Phi.T).T      # (the constant is part of the matrix)
    else:
        hx, hz, hc = pack_terms(n, ham.terms)
        hx, hz, hc = [int(x) for x in hx], [int(z) for z in hz], list(hc)
        Sigma = np.array([masks.apply_pauli_sum(v, hx, hz, hc) for v in Phi]) + complex(ham.constant_coeff) * Phi
    return Phi, np.asarray(Sigma)


def matrices(psi, n, ops, ham):
    """-> (S, G or None, rows)"""
    psi = np.asarray(psi, np.complex128)
    Phi, Sigma = phi_sigma(psi, n, ops, ham)
    S = Phi.conj() @ Phi.T
    G = None if Sigma is None else Phi.conj() @ Sigma.T
    return S, G, expected_rows(psi, n, ops)


def s_bound(n, ops):
    a = weights(n, ops)
    return 1e-12 * np.outer(a, a)


def g_bound(n, ops, ham):
    a = weights(n, ops)
    return 1e-10 * h_norm1(ham) * np.outer(a, a)


def _within(got, want, bound):
    d = got - want
    return bool(np.all(np.abs(d.real) <= bound) and np.all(np.abs(d.imag) <= bound))


def compare(what, S, G, want_S, want_G, n, ops, ham):
    """S and the RAW G against the checker, element by element; prints the figures before it asserts"""
    sb = s_bound(n, ops)
    tiny = np.finfo(float).tiny
    print(f"{what}: max |dS| / bound = {np.max(np.abs(S - want_S) / np.maximum(sb, tiny)):.3e}")
    assert _within(S, want_S, sb), what
    if G is not None:
        gb = g_bound(n, ops, ham)
        print(f"{what}: max |dG| / bound = {np.max(np.abs(G - want_G) / np.maximum(gb, tiny)):.3e}, "
              f"max |G - G^H| / bound = {np.max(np.abs(G - G.conj().T) / np.maximum(gb, tiny)):.3e}")
        assert _within(G, want_G, gb), what
        assert _within(G, G.conj().T, gb), what


# ---- case builders --------------------------------------------------------------------------------------------------------------------
def identity(n):
    return Hamiltonian(n, [], 1.0)


def random_pool(rng, n, m):
    """m operators of 1 - 6 random strings with complex coefficients, operator 0 the identity"""
    ops = [identity(n)]
    for _ in range(1, m):
        terms = []
        for _ in range(int(rng.integers(1, 7))):
            op, qs = util.random_string(rng, n)
            terms.append(Term(complex(rng.normal(), rng.normal()), op, qs))
        ops.append(Hamiltonian(n, terms, do_clean_up=False))
    return ops


def hamiltonian_with_groups(rng, n, ngroups, terms_in_first=1):
    """a Hamiltonian with exactly ``ngroups`` distinct x masks, x = 0 among them (ngroups = 1: diagonal only), ``terms_in_first``
    strings in the first non-diagonal group (the diagonal one when it is alone) that differ in X <-> Y and Z only, the other groups
    one string each, non-zero constant"""
    assert 1 <= ngroups <= (1 << n)
    terms, seen = [], set()
    xs = [0] + [int(x) for x in rng.permutation(np.arange(1, 1 << n))[:ngroups - 1]]
    for k, x in enumerate(xs):
        want = terms_in_first if k == min(1, len(xs) - 1) else 1
        made = 0
        while made < want:
            z = int(rng.integers(0, 1 << n))
            if (x, z) in seen or (x == 0 and z == 0):
                continue
            seen.add((x, z))
            qs = [q for q in range(n) if ((x | z) >> (n - 1 - q)) & 1]
            op = "".join("Y" if (x >> (n - 1 - q)) & 1 and (z >> (n - 1 - q)) & 1 else "X" if (x >> (n - 1 - q)) & 1 else "Z" for q in qs)
            terms.append(Term(float(rng.normal()), op, qs))
            made += 1
    ham = Hamiltonian(n, terms, float(rng.normal()), do_clean_up=False)
    assert len({pack(n, t)[0] for t in ham.terms}) == ngroups
    return ham


def pack(n, term):
    return masks.pack_pauli(n, term.op, term.qbits)


def sector_indices(n, hf):
    """register indices with the (N_alpha, N_beta) of the determinant ``hf`` (qubit q = index bit n-1-q, even qubits alpha)"""
    amask = sum(1 << (n - 1 - q) for q in range(0, n, 2))
    bmask = sum(1 << (n - 1 - q) for q in range(1, n, 2))
    na, nb = bin(hf & amask).count("1"), bin(hf & bmask).count("1")
    return np.array([i for i in range(1 << n) if bin(i & amask).count("1") == na and bin(i & bmask).count("1") == nb])


class Molecule:
    """synthetic_molecule(n_spatial, n_occ, seed) with the spectrum of the Hamiltonian's (N_alpha, N_beta) block of the reference
    determinant from dense numpy, and psi = its lowest eigenvector embedded in the register"""

    def __init__(self, n_spatial, n_occ, seed):
        self.n_spatial, self.n_occ = n_spatial, n_occ
        self.ham, self.gens, self.hf = fermion.synthetic_molecule(n_spatial, n_occ, seed)
        self.n = 2 * n_spatial
        self.sector = sector_indices(self.n, self.hf)
        hmat = self.ham.get_matrix(sparse=True).tocsr()[self.sector][:, self.sector].toarray()
        assert np.abs(hmat - hmat.conj().T).max() < 1e-13
        self.block_energies, vecs = np.linalg.eigh(hmat)
        self.psi = np.zeros(1 << self.n, np.complex128)
        self.psi[self.sector] = vecs[:, 0]

    def pool(self, deexcitations=False):
        from openvqe_amd import excited
        return excited.excitation_operators(self.n_spatial, self.n_occ, deexcitations=deexcitations, identity=True)


def assert_spectrum_gap(S):
    """the condition under which the rank cannot depend on rounding: no eigenvalue of S between 1e-13 and 1e-5 of the largest"""
    w = np.linalg.eigvalsh(S)
    ratio = w / w[-1]
    assert not np.any((ratio > 1e-13) & (ratio < 1e-5)), ratio
    return ratio
