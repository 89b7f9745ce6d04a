"""TEST INFRASTRUCTURE ONLY — checker of the subspace-expansion matrices (ovqe_subspace_matrices) and the case builders of
tests/test_subspace_cases.py / tests/test_gpu_subspace.py / tests/test_gpu_subspace_edges.py, with the tolerance every GPU result is
held to, and the plan of a call (sub::plan) restated in Python with the table of the boundary cases.

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


# ---- the plan of a call, restated (openvqe_amd/csrc/sv_subspace_host.hpp: sub::plan; the two grids: subspace_host.inc) ------------------
GRAM_BLOCK, GRAM_TILE_ROWS, GRAM_MAX_SLICES = 64, 16, 256
SIGMA_ROW_TILE, SIGMA_MAX_BLOCKS = 4, 4
MI355X_CUS = 256


def plan(rows, m, with_h, num_cus):
    """sub::plan in Python, the fields tests/cpu/subspace_plan_check.cpp prints in its ``boundary`` mode, plus the two grid sizes of
    subspace_host.inc (``sigma_grid``: workgroups in x of the sigma launch, ``expand_grid``: workgroups of the expand launch; both 0
    when the kernel is not launched)"""
    up = lambda a, b: -(-a // b)
    nb = up(m, GRAM_BLOCK)
    mb = nb * GRAM_BLOCK
    s_pairs = nb * (nb + 1) // 2
    tiles = max(1, up(rows, GRAM_TILE_ROWS))
    sized_for = s_pairs + nb * nb                    # (the slices are sized for a call with h_out either way)
    want = up(4 * max(num_cus, 1), sized_for)
    slices = max(1, min(want, tiles, GRAM_MAX_SLICES))
    slice_rows = up(tiles, slices) * GRAM_TILE_ROWS
    slices = up(tiles * GRAM_TILE_ROWS, slice_rows)
    sigma_blocks = SIGMA_MAX_BLOCKS if nb >= SIGMA_MAX_BLOCKS else 2 if nb >= 2 else 1
    row_tiles = up(rows, SIGMA_ROW_TILE)
    return dict(rows=rows, m=m, with_h=int(bool(with_h)), nb=nb, mb=mb, wpad=2 * mb if with_h else mb,
                pairs=s_pairs + (nb * nb if with_h else 0), slices=slices, slice_rows=slice_rows, sigma_blocks=sigma_blocks,
                col_groups=up(nb, sigma_blocks), row_tiles=row_tiles,
                sigma_grid=min(row_tiles, num_cus * 32) if with_h and rows else 0,
                expand_grid=min(up(rows * mb, 256), num_cus * 16) if rows else 0)


PLAN_FIELDS = ("rows", "m", "with_h", "nb", "mb", "wpad", "pairs", "slices", "slice_rows", "sigma_blocks", "col_groups", "row_tiles")


def check_info_against_plan(info, rows, m, with_h, num_cus=MI355X_CUS):
    """the path figures of ``subspace_info()`` against the restated plan; -> the plan"""
    p = plan(rows, m, with_h, num_cus)
    ran_sigma = bool(with_h and rows)
    want = dict(m=m, rows=rows, block_pairs=p["pairs"], slices=p["slices"], slice_rows=p["slice_rows"],
                sigma_blocks=p["sigma_blocks"] if ran_sigma else 0, sigma_col_groups=p["col_groups"] if ran_sigma else 0,
                sigma_grid=p["sigma_grid"], expand_grid=p["expand_grid"], store_bytes=rows * p["wpad"] * 16,
                expand_launches=int(rows > 0), sigma_launches=int(ran_sigma), gram_launches=1)
    got = {k: info[k] for k in want}
    assert got == want, (got, want)
    return p


# ---- builders of the boundary cases (tests/test_gpu_subspace_edges.py) --------------------------------------------------------------------
def term_from_masks(n, coeff, x, z):
    """the Pauli string with index-space masks (x, z): X where only x is set, Z where only z, Y where both"""
    qs = [q for q in range(n) if ((x | z) >> (n - 1 - q)) & 1]
    op = "".join("Y" if (x >> (n - 1 - q)) & 1 and (z >> (n - 1 - q)) & 1 else "X" if (x >> (n - 1 - q)) & 1 else "Z" for q in qs)
    return Term(coeff, op, qs)


def xor_span(xs):
    """all XOR combinations of the masks in ``xs`` (0 included), ascending"""
    span = {0}
    for x in xs:
        span |= {s ^ int(x) for s in span}
    return sorted(span)


def closed_support_state(rng, n, rows, xs):
    """a normalised complex state whose support has exactly ``rows`` indices and is closed under every mask in ``xs``: ``rows / |V|``
    cosets of the span V of the masks, drawn without replacement.  With a pool whose x masks are those (and 0), R is the support."""
    span = np.array(xor_span(xs), np.int64)
    assert rows % span.shape[0] == 0 and 0 < rows <= (1 << n), (rows, span.shape[0])
    idx = np.arange(1 << n, dtype=np.int64)
    reps = idx[np.min(idx[:, None] ^ span[None, :], axis=1) == idx] if span.shape[0] > 1 else idx    # the least index of each coset
    chosen = rng.choice(reps, rows // span.shape[0], replace=False)
    support = np.unique((chosen[:, None] ^ span[None, :]).reshape(-1))
    assert support.shape[0] == rows
    psi = np.zeros(1 << n, np.complex128)
    psi[support] = rng.normal(size=rows) + 1j * rng.normal(size=rows)
    assert np.all(psi[support] != 0)
    return psi / np.linalg.norm(psi)


def pool_with_x(rng, n, m, xs):
    """m operators, operator 0 the identity, the others 1 - 4 strings each with complex coefficients, x masks from ``xs`` only (taken in
    turn, so that all of them are used: asserted) and random z masks"""
    xs = [int(x) for x in xs]
    ops, used, turn = [identity(n)], {0}, 0
    for _ in range(1, m):
        terms, seen, want = [], set(), max(int(rng.integers(1, 5)), -(-len(xs) // (m - 1)))
        while len(terms) < want:
            x = xs[turn % len(xs)]
            z = int(rng.integers(0, 1 << n))
            if (x, z) in seen or (x == 0 and z == 0):
                continue
            turn += 1
            seen.add((x, z))
            used.add(x)
            terms.append(term_from_masks(n, complex(rng.normal(), rng.normal()), x, z))
        ops.append(Hamiltonian(n, terms, do_clean_up=False))
    assert used == set(xs) | {0}, (sorted(used), sorted(xs))
    return ops


def small_hamiltonian(rng, n, xs, constant=0.375):
    """one string per x mask in ``xs`` (random z, real coefficient): a Hamiltonian whose x-groups the caller chooses"""
    terms = []
    for x in xs:
        z = int(rng.integers(1, 1 << n))
        terms.append(term_from_masks(n, float(rng.normal()), int(x), z))
    return Hamiltonian(n, terms, constant, do_clean_up=False)


def cancelling_pairs(n):
    return [(q, q + 1) for q in range(0, n - 1, 2)]


def cancelling_hamiltonian(n, constant=0.25, ulp=False):
    """constant + sum over the neighbouring pairs (0, 1), (2, 3), ... of c (XX) + c' (YY), c = 1/2: each pair is ONE x-group whose
    coefficient D_g(k) = c - c' (-1)^{k_q + k_q+1} is c - c' wherever the two bits of the pair agree — exactly zero for c' = c, and
    with ``ulp`` (c' the double above 1/2) a residue of 1.1e-16, far below the group's 64 eps (c + c') = 1.4e-14 that
    group_coeff_snap treats as zero.  On the rows where every pair agrees no group is live and sigma is constant * phi."""
    c2 = float(np.nextafter(0.5, 1.0)) if ulp else 0.5
    terms = []
    for q, r in cancelling_pairs(n):
        terms += [Term(0.5, "XX", [q, r]), Term(c2, "YY", [q, r])]
    return Hamiltonian(n, terms, constant, do_clean_up=False)


def agreeing_indices(n):
    """register indices on which the two bits of every pair of ``cancelling_pairs`` agree"""
    bit = lambda q: n - 1 - q
    return np.array([i for i in range(1 << n) if all(((i >> bit(q)) ^ (i >> bit(r))) & 1 == 0 for q, r in cancelling_pairs(n))])


def group_coefficient(n, ham, x, k):
    """D_g(k) = sum over the strings of ``ham`` with x mask ``x`` of c_t i^ny (-1)^{popcount(k & z_t)}, summed in the order given"""
    d = 0.0
    for t in ham.terms:
        tx, tz = pack(n, t)
        if tx == x:
            d = d + complex(t.coeff) * 1j ** (bin(tx & tz).count("1") % 4) * (-1.0) ** bin(k & tz).count("1")
    return d


def handle_group_order(n, ham):
    """the x masks of a Hamiltonian in the order of the handle's group list: ascending (build_groups sorts the terms by x)"""
    return sorted({pack(n, t)[0] for t in ham.terms})


def one_live_group(n, ngroups, which):
    """-> (ham, psi, (a, b, c)).  The Hamiltonian has the x-groups 1 .. ngroups (one string each), so position p of the handle's group
    list is x = p + 1.  psi lives on a = 0, b = which + 1 and c, a third index with a bit above every x mask: under a pool of diagonal
    operators R = {a, b, c}; on rows a and b exactly the group at position ``which`` has its partner inside R, on row c none has."""
    assert 0 <= which < ngroups and ngroups < (1 << (n - 1))
    rng = np.random.default_rng(1000 * ngroups + which)
    ham = small_hamiltonian(rng, n, range(1, ngroups + 1), constant=-0.625)
    a, b, c = 0, which + 1, (1 << (n - 1)) | 5
    psi = np.zeros(1 << n, np.complex128)
    psi[[a, b, c]] = rng.normal(size=3) + 1j * rng.normal(size=3)
    return ham, psi / np.linalg.norm(psi), (a, b, c)


def live_groups(n, ham, R, row):
    """positions in the handle's group order of the x-groups with a partner of ``row`` inside R and a non-zero coefficient there"""
    R = set(int(i) for i in R)
    return [p for p, x in enumerate(handle_group_order(n, ham)) if (row ^ x) in R and group_coefficient(n, ham, x, row ^ x) != 0]


# ---- the boundary cases by name: (qubits, rows, m, with_h) and the branch of the launch code each is named for, as a predicate on the
# plan at 256 CUs (tests/test_subspace_cases.py checks the table on the CPU, tests/test_gpu_subspace_edges.py runs the cases) -----------
WIDTHS = (192, 193, 255, 256, 257, 320, 321)
WIDTH_DENSE_N, WIDTH_SPARSE_N, WIDTH_SPARSE_ROWS = 7, 8, 42


def width_branch(m):
    """the sigma instantiation and its column groups for a pool of m operators: NB = 4 from 193 on, two groups from 257 to 512, the
    live blocks of the last group (4 = full)"""
    nb = -(-m // 64)
    return lambda p: (p["nb"] == nb and p["sigma_blocks"] == (4 if m >= 193 else 2) and p["col_groups"] == (2 if m >= 257 or m == 192 else 1)
                      and p["mb"] - m == (64 - m % 64) % 64)


EDGE_CASES = {}
for _m in WIDTHS:
    EDGE_CASES[f"width dense m={_m}"] = ((WIDTH_DENSE_N, 1 << WIDTH_DENSE_N, _m, True), width_branch(_m))
    EDGE_CASES[f"width sparse m={_m}"] = ((WIDTH_SPARSE_N, WIDTH_SPARSE_ROWS, _m, True), width_branch(_m))
EDGE_CASES.update({
    "width dense m=257 S only": ((WIDTH_DENSE_N, 128, 257, False), lambda p: p["nb"] == 5 and p["wpad"] == 320 and p["sigma_grid"] == 0),
    "width sparse m=257 S only": ((WIDTH_SPARSE_N, WIDTH_SPARSE_ROWS, 257, False), lambda p: p["nb"] == 5 and p["wpad"] == 320 and p["sigma_grid"] == 0),
    "gram two tiles": ((9, 512, 257, True), lambda p: p["pairs"] == 40 and p["slice_rows"] == 32 and p["slices"] == 16),
    "gram slice cap": ((13, 8192, 2, True), lambda p: p["slices"] == 256 and p["slice_rows"] == 32),
    "gram short last slice": ((13, 4101, 3, True), lambda p: p["slice_rows"] == 32 and p["slices"] == 129 and 4101 - 128 * 32 == 5),
    "gram rows % 16 == 1": ((13, 4113, 3, True), lambda p: p["rows"] % 16 == 1 and p["slice_rows"] == 32 and p["slices"] == 129
                            and p["rows"] - 128 * 32 == 17),
    "gram rows == 16 slices": ((10, 592, 3, True), lambda p: p["rows"] == 16 * p["slices"] and p["slice_rows"] == 16),
    "stride dense": ((16, 1 << 16, 3, True), lambda p: p["sigma_grid"] * 4 < p["rows"] and p["expand_grid"] * 256 < p["rows"] * 64
                     and p["rows"] * p["wpad"] * 16 == 128 << 20),
    "stride sparse": ((16, 40000, 3, True), lambda p: p["sigma_grid"] * 4 < p["rows"] and p["expand_grid"] * 256 < p["rows"] * 64),
    "zero rows": ((6, 0, 5, True), lambda p: p["slices"] == 1 and p["sigma_grid"] == 0 and p["expand_grid"] == 0),
    "handle dense m=257": ((10, 1024, 257, True), lambda p: p["sigma_blocks"] == 4 and p["col_groups"] == 2 and p["slice_rows"] == 48),
    "handle sparse m=3": ((10, 30, 3, True), lambda p: p["sigma_blocks"] == 1 and p["wpad"] == 128 and p["slices"] == 2),
    "handle sparse m=3 S only": ((10, 30, 3, False), lambda p: p["wpad"] == 64 and p["slices"] == 2),
    "handle dense m=65 S only": ((10, 1024, 65, False), lambda p: p["wpad"] == 128 and p["nb"] == 2),
    "handle dense m=65": ((10, 1024, 65, True), lambda p: p["wpad"] == 256 and p["sigma_blocks"] == 2 and p["col_groups"] == 1),
})


def edge_plan(name, num_cus=MI355X_CUS):
    (n, rows, m, with_h), branch = EDGE_CASES[name]
    return plan(rows, m, with_h, num_cus), branch
