"""TEST INFRASTRUCTURE ONLY — programs, Hamiltonians and the exact gradient reference of tests/test_sector_cases.py (CPU) and
tests/test_gpu_sector_forms.py (GPU), which pin the kernel forms of the sector path (openvqe_amd/csrc/sv_sector.hpp, sector_host.inc).

THE GRADIENT REFERENCE (``support_gradient``) is the reverse-mode pass of ``oracle.masks.ucc_energy_gradient`` restricted to the
support S of the program's states (``tests.util.support_closure``), complex128, no finite differences.  It starts from the C
oracle's final state and lambda = H psi on S and walks the program backwards RUN BY RUN: consecutive rotations with one x mask
and odd Y counts commute, and on the pair (i, i ^ x) the run is one rotation with the matrix [[0, conj(A)], [A, 0]],
A = sum_r phi_r <i ^ x|P_r|i>.  Pairs with one member outside S are left out, which is exact: S is closed under every pair a run
moves amplitude across for generic angles, and on the other pairs A — and with it the summed derivative of every parameter —
vanishes identically.  tests/test_sector_cases.py holds it against the dense-register pass and against central differences of
the C oracle.

THE COUNTED-MAGNITUDE HAMILTONIAN (``counted_hamiltonian``) is a sum of X-only strings c_x X^x with pairwise distinct |c_x|, every x
of weight >= 3 inside ``COUNTED_BITS`` = 13 fixed index bits (one <H> sweep with "sector_h_bits" = 13 covers them all), and one
diagonal term.  Every matrix element of the group x is c_x, so the sweep's dictionary holds one magnitude per x-group that connects
two members of the support, and one more (``COUNTED_DICT_EXTRA``).  It runs on
``counted_case``: the support is the 13-bit strings without (bit 11 and bit 12) on 16 qubits — 6144 amplitudes in ONE <H> tile
(a full 13-bit coset would be 8192, above the 7600 the <H> kernels hold in LDS, and the tile bits would be lowered) — and every
13-bit mask connects two of its members."""
import functools

import numpy as np

from openvqe_amd import fermion
from openvqe_amd.backend import compile_ucc_program
from openvqe_amd.operators import Hamiltonian, Term
from tests import util


# ---- programs ---------------------------------------------------------------------------------------------------------------------------
class Case:
    """a rotation program with its Hamiltonian: packed arrays, support, oracle energies / states and reference gradients, cached"""

    def __init__(self, name, n, ham, gens, hf):
        self.name, self.n, self.ham, self.gens, self.hf = name, n, ham, gens, int(hf)
        self.rx, self.rz, self.rc, self.pidx, self.K = compile_ucc_program(n, gens)
        hx, hz, hc = ham.packed()
        assert np.abs(hc.imag).max(initial=0.0) == 0.0
        self.hx, self.hz, self.hc = hx, hz, np.ascontiguousarray(hc.real)
        self.l1 = float(np.abs(self.hc).sum())
        self.bound = max(1.0, self.l1)
        self._cache = {}

    @functools.cached_property
    def support(self):
        return util.support_closure(self.hf, self.rx, self.rz, self.rc, self.pidx)

    def thetas(self, count=3, scale=0.3, seed=0):
        """``count`` parameter vectors, the LAST one zero (|hf> itself: every rotation is the identity)"""
        rng = np.random.default_rng(1000 + seed)
        return [rng.uniform(-scale, scale, self.K) for _ in range(count - 1)] + [np.zeros(self.K)]

    def oracle(self, theta):
        """(energy, final state) of the C oracle"""
        from oracle import cref
        key = ("oracle", np.asarray(theta, np.float64).tobytes())
        if key not in self._cache:
            self._cache[key] = cref.ucc_energy(self.n, self.hf, self.rx, self.rz, self.rc, self.pidx, theta, self.hx, self.hz, self.hc,
                                               self.ham.constant_coeff, 0)
        return self._cache[key]

    def energy(self, theta):
        return self.oracle(theta)[0]

    def gradient(self, theta):
        """(energy, grad[K]) of the support-only adjoint pass from the oracle's final state"""
        key = ("gradient", np.asarray(theta, np.float64).tobytes())
        if key not in self._cache:
            self._cache[key] = support_gradient(self.support, self.rx, self.rz, self.rc, self.pidx, theta, self.hx, self.hz, self.hc,
                                                self.ham.constant_coeff, self.oracle(theta)[1])
        return self._cache[key]


@functools.lru_cache(maxsize=None)
def molecule(m, o, seed=None, singles_only=False, one_body=False):
    """``fermion.synthetic_molecule`` with its UCCSD generators, or with the single excitations alone (2 o (m - o) generators of two
    strings each: the support is still the whole (o alpha, o beta) sector); ``one_body``: the Hamiltonian of the one-electron
    integrals alone (a few hundred strings instead of ten thousand at 20 qubits: the checker's time goes into the circuit)"""
    seed = 100 * m + o if seed is None else seed
    ham, gens, hf = fermion.synthetic_molecule(m, o, seed=seed)
    if one_body:
        h, g = fermion.synthetic_integrals(m, seed)
        ham = fermion.jw_molecular_hamiltonian(*fermion.spin_orbital_integrals(h, 0.0 * g), 0.25)
    if singles_only:
        gens = gens[:2 * o * (m - o)]
        assert all(len(g.terms) == 2 for g in gens)
    return Case(f"{'singles' if singles_only else 'uccsd'}({m},{o}){' one-body H' if one_body else ''}", 2 * m, ham, gens, hf)


# ---- the counted-magnitude Hamiltonian and its program ------------------------------------------------------------------------------------
COUNTED_N, COUNTED_BITS = 16, 13
COUNTED_SUPPORT = 3 * (1 << 11)        # 13-bit strings without (bit 11 and bit 12)


def counted_generators(n=COUNTED_N, bits=COUNTED_BITS):
    """single-string rotations (one Y each, so the amplitudes stay real) and one two-string excitation: Y on the index bits
    0 .. bits - 2, the excitation bit (bits - 2) -> bit (bits - 1), then XY / YX strings on neighbouring bits so that every pair of
    the support is rotated by several parameters.  Qubit q is index bit n - 1 - q."""
    from tests.subspace_cases import term_from_masks
    one = lambda coeff, x, z: Hamiltonian(n, [term_from_masks(n, float(coeff), x, z)], do_clean_up=False)
    gens = [one(1.0, 1 << b, 1 << b) for b in range(bits - 1)]
    xs, zs, cs = util.pattern_excitation([bits - 2], [bits - 1])
    gens.append(Hamiltonian(n, [term_from_masks(n, float(c), x, z) for x, z, c in zip(xs, zs, cs)], do_clean_up=False))
    for b in range(0, bits - 3, 2):                     # x masks inside the free bits: the support does not grow
        gens.append(one(0.7 + 0.05 * b, 3 << b, (1 << b) | (1 << 7 if b not in (6, 7) else 1 << 9)))       # Y X, and a Z elsewhere
    for b in range(1, bits - 3, 3):
        gens.append(one(-0.9 + 0.04 * b, 3 << b, 2 << b))                                                  # X Y
    return gens


def counted_masks(bits=COUNTED_BITS):
    """the masks of weight >= 3 inside the low ``bits`` index bits, in a fixed shuffled order (8100 for 13 bits)"""
    xs = np.array([x for x in range(1 << bits) if bin(x).count("1") >= 3], np.uint64)
    return xs[np.random.default_rng(13).permutation(len(xs))]


def connected(support, x):
    """some member i of the support has i ^ x in the support too"""
    j = support ^ np.uint64(x)
    pos = np.minimum(np.searchsorted(support, j), len(support) - 1)
    return bool(np.any(support[pos] == j))


def counted_hamiltonian(groups, support, n=COUNTED_N, bits=COUNTED_BITS, diagonal=0.3125, constant=-0.75):
    """``groups`` X-only strings on masks of ``counted_masks`` that connect members of ``support``, |c_x| = 0.5 + k / 16384 for the k-th
    (pairwise distinct, all below 1, none equal to |diagonal|), signs alternating in threes; one Z string; a constant.
    -> (Hamiltonian, kept masks)"""
    kept = []
    for x in counted_masks(bits):
        if len(kept) == groups:
            break
        if connected(support, int(x)):
            kept.append(int(x))
    assert len(kept) == groups, (len(kept), groups)
    terms = []
    for k, x in enumerate(kept):
        qs = [n - 1 - b for b in range(bits - 1, -1, -1) if (x >> b) & 1]
        terms.append(Term((0.5 + k / 16384.0) * (-1.0 if k % 3 == 2 else 1.0), "X" * len(qs), qs))
    terms.append(Term(float(diagonal), "Z", [n - 1 - 5]))
    return Hamiltonian(n, terms, constant, do_clean_up=False), kept


@functools.lru_cache(maxsize=None)
def counted_case(groups):
    gens = counted_generators()
    hf = 1 << 14                                             # (a bit outside the 13: the tile of the support is not tile 0)
    rx, rz, rc, pidx, _ = compile_ucc_program(COUNTED_N, gens)
    support = util.support_closure(hf, rx, rz, rc, pidx)
    ham, kept = counted_hamiltonian(groups, support)
    case = Case(f"counted({groups})", COUNTED_N, ham, gens, hf)
    case.kept = kept
    return case


@functools.lru_cache(maxsize=None)
def many_pattern_case(strings=6, n=14):
    """ONE generator of ``strings`` strings with generic coefficients on one x mask of weight 5 (index bits 0..4; Y on an odd number of
    them, nothing outside): the run fuses into a table op whose rotation angle differs on all 16 settings of the four non-pivot
    bits — 16 patterns, more than the 8 a 14-bit slot field leaves room for — behind Y rotations that spread the support over the
    bits 0..4 and 6..9 (512 of 2^14 amplitudes); a Hamiltonian of 60 random strings of weight <= 4"""
    from tests.subspace_cases import term_from_masks
    one = lambda coeff, x, z: Hamiltonian(n, [term_from_masks(n, float(coeff), x, z)], do_clean_up=False)
    rng = np.random.default_rng(1313)
    gens = [one(1.0, 1 << b, 1 << b) for b in (0, 1, 2, 3, 4, 6, 7, 8, 9)]
    odd = [z for z in range(32) if bin(z).count("1") & 1]
    picks = rng.choice(len(odd), strings, replace=False)
    gens.append(Hamiltonian(n, [term_from_masks(n, float(rng.uniform(0.2, 1.0)), 0x1f, odd[k]) for k in picks], do_clean_up=False))
    seen, terms = set(), []
    while len(terms) < 60:
        op, qs = util.random_string(rng, n, 1, 4)
        if (op, tuple(qs)) not in seen and op.count("Y") % 2 == 0:
            seen.add((op, tuple(qs)))
            terms.append(Term(float(rng.normal()), op, qs))
    return Case(f"patterns({strings})", n, Hamiltonian(n, terms, 0.25), gens, 1 << 11)


# GROUP COUNTS of the coding boundaries: X groups -> entries the sweep's dictionary reports (ovqe_program_info "sector_h_max_dict").
# Measured on the MI355X: the dictionary of the sweep reports groups + 1 entries — the magnitudes of the X groups and one more, the
# diagonal term's or the zero of padded rows (the count does not tell which of the two is kept outside the coded stream).
COUNTED_DICT_EXTRA = 1
COUNTED_GROUPS = {1023: 1023 - COUNTED_DICT_EXTRA, 1024: 1024 - COUNTED_DICT_EXTRA, 4096: 4096 - COUNTED_DICT_EXTRA,
                  4097: 4097 - COUNTED_DICT_EXTRA}


# ---- lambda = H psi and the adjoint pass on the support -----------------------------------------------------------------------------------
def _parity(v):
    v = v.copy()
    for s in (32, 16, 8, 4, 2, 1):
        v ^= v >> np.uint64(s)
    return (v & np.uint64(1)).astype(np.float64)


def _partners(support, x):
    """(rows, positions of their partners) for the members i of the support whose partner i ^ x is a member too"""
    j = support ^ np.uint64(x)
    pos = np.minimum(np.searchsorted(support, j), len(support) - 1)
    rows = np.flatnonzero(support[pos] == j)
    return rows, pos[rows]


def apply_on_support(support, vec, hx, hz, hc):
    """(H vec) restricted to the support, vec given on the support: (P v)_i = i^ny (-1)^{|(i ^ x) & z|} v_{i ^ x}"""
    out = np.zeros(len(support), np.complex128)
    order = np.argsort(np.asarray(hx, np.uint64), kind="stable")
    xs, zs, cs = np.asarray(hx, np.uint64)[order], np.asarray(hz, np.uint64)[order], np.asarray(hc)[order]
    t = 0
    while t < len(xs):
        e = t
        while e < len(xs) and xs[e] == xs[t]:
            e += 1
        x = int(xs[t])
        rows, part = _partners(support, x)
        if len(rows):
            src = support[part]
            coeff = np.zeros(len(rows), np.complex128)
            for k in range(t, e):
                z = int(zs[k])
                coeff += complex(cs[k]) * (1j) ** (bin(x & z).count("1") % 4) * (1.0 - 2.0 * _parity(src & np.uint64(z)))
            out[rows] += coeff * vec[part]
        t = e
    return out


def support_gradient(support, rx, rz, rc, pidx, theta, hx, hz, hc, constant, psi_final):
    """E and dE/dtheta by the adjoint pass on the support, from the final state ``psi_final`` (full register) -> (E, grad[K]).
    Asserts that the final state lives on the support."""
    theta = np.asarray(theta, np.float64)
    support = np.asarray(support, np.uint64)
    psi_final = np.asarray(psi_final, np.complex128)
    outside = np.ones(psi_final.shape[0], bool)
    outside[support.astype(np.int64)] = False
    assert np.abs(psi_final[outside]).max(initial=0.0) < 1e-13, "the oracle's state leaves the support"
    psi = psi_final[support.astype(np.int64)].copy()
    lam = apply_on_support(support, psi, hx, hz, hc)
    energy = float(np.vdot(psi, lam).real) + float(np.real(constant))
    grad = np.zeros(len(theta), np.float64)
    R = len(rx)
    runs, r = [], 0
    while r < R:
        e = r
        while e < R and int(rx[e]) == int(rx[r]):
            e += 1
        runs.append((r, e))
        r = e
    geometry = {}
    for r, e in reversed(runs):
        x = int(rx[r])
        if x == 0:                                            # diagonal strings: a phase on every amplitude, no derivative of a real energy... kept general
            for t in range(r, e):
                sign = 1.0 - 2.0 * _parity(support & np.uint64(int(rz[t])))
                if int(pidx[t]) >= 0:
                    grad[int(pidx[t])] += 2.0 * float(rc[t]) * float(np.vdot(lam, sign * psi).imag)
                phase = np.exp(1j * float(rc[t]) * float(theta[int(pidx[t])]) * sign)
                psi, lam = phase * psi, phase * lam
            continue
        if x not in geometry:
            pivot = np.uint64(1 << (x.bit_length() - 1))
            rows, part = _partners(support, x)
            low = (support[rows] & pivot) == 0
            geometry[x] = (rows[low], part[low])
        p0, p1 = geometry[x]
        i0 = support[p0]
        assert e - r == 1 or all(bin(x & int(rz[t])).count("1") & 1 for t in range(r, e)), "a run of strings that do not commute"
        A = np.zeros(len(p0), np.complex128)
        psi0, psi1, lam0, lam1 = psi[p0], psi[p1], lam[p0], lam[p1]
        for t in range(r, e):
            z = int(rz[t])
            a = (1j) ** (bin(x & z).count("1") % 4) * (1.0 - 2.0 * _parity(i0 & np.uint64(z)))       # <i0 ^ x| P |i0>
            if int(pidx[t]) >= 0:
                m = np.vdot(lam1, a * psi0) + np.vdot(lam0, np.conj(a) * psi1)
                grad[int(pidx[t])] += 2.0 * float(rc[t]) * float(m.imag)
                A += float(rc[t]) * float(theta[int(pidx[t])]) * a
        rho = np.abs(A)
        c = np.cos(rho)
        s = np.where(rho > 0, np.sin(rho) / np.where(rho > 0, rho, 1.0), 1.0)
        psi[p0], psi[p1] = c * psi0 + 1j * s * np.conj(A) * psi1, c * psi1 + 1j * s * A * psi0       # exp(+i M): the run undone
        lam[p0], lam[p1] = c * lam0 + 1j * s * np.conj(A) * lam1, c * lam1 + 1j * s * A * lam0
    return energy, grad
