"""TEST INFRASTRUCTURE ONLY — the three batched gradient calls (ovqe_energy_gradient_batch, ovqe_deflated_gradient_batch,
ovqe_spread_gradient_batch) where their compact path ends: the case builders of tests/test_stream_cases.py / tests/test_gpu_stream_batches.py,
the constants the cases are derived from, and a Python restatement of the cover rule of the Pauli-sum application (grow_tile_set in
csrc/sv_cover_host.hpp as build_ham_tiles in csrc/tile_host.inc calls it).

No new mathematics: the checkers are ``oracle.masks.ucc_energy_gradient`` (``gradbatch_cases.Case.want``), ``deflation_cases.case_want``
and ``spread_cases.case_want``; the bounds are those modules'.

The constants, and what follows from each (a constant that moves takes the sizes named beside it along):
  COMPACT_MAX_QUBITS = 16   the test ``n_local > 16`` of run_sparse_gradient / run_grad_batch / run_vqd_batch / run_spread_batch:
                            ``boundary_pair`` sits at 16 | 17;
  TILE_BITS = 11            tiles of the Pauli-sum application below 25 qubits (tile_bits, ovqe_sv.hip), TILE_LOW = 2 lowest index bits in
                            every tile (HAM_TILE_LOW): a Hamiltonian whose x masks span more than 11 bits needs two sweeps;
  APPLY_MIN_TILES = 256     apply_hamiltonian takes k_tile_apply from 256 tiles on: 2^(11 + 8) amplitudes, 19 qubits — ``TILED_FROM``;
  REDUCE_BLOCKS x REDUCE_THREADS = 2048 x 256   the cap of reduce_blocks: a lane of the vector kernels makes a second trip of its
                            grid-stride loop from 2^19 + 1 amplitudes on, every lane from 2^20 — ``SECOND_TRIP_FROM`` = 20 qubits;
  DEFLATE_CHUNK = 4, DEFLATE_MAX = 32   vectors per pass of k_deflate_dots / k_deflate_axpy, vectors a handle holds: J = 1 a remainder alone,
                            4 one full pass, 5 a full pass and a remainder of one, 32 eight full passes and slots 0 to 31 of d_result."""
import numpy as np

from tests import deflation_cases as dc
from tests import gradbatch_cases as gc
from tests import hessian_cases

COMPACT_MAX_QUBITS = 16
TILE_BITS, TILE_LOW = 11, 2
APPLY_MIN_TILES = 256
REDUCE_BLOCKS, REDUCE_THREADS = 2048, 256
DEFLATE_CHUNK, DEFLATE_MAX = 4, 32
TILED_FROM = TILE_BITS + (APPLY_MIN_TILES - 1).bit_length()                        # 19 qubits
SECOND_TRIP_FROM = (REDUCE_BLOCKS * REDUCE_THREADS).bit_length()                   # 20 qubits: 2^20 = two trips of 2^19 lanes
NO_TILES = 1 << 30                                                                 # "apply_min_tiles": never the tiled form


def reduce_blocks(namps):
    """reduce_blocks (ovqe_sv.hip): workgroups of 256 of every vector kernel"""
    return min(REDUCE_BLOCKS, max(1, (namps + REDUCE_THREADS - 1) // REDUCE_THREADS))


def trips(n):
    """grid-stride trips of a lane of a vector kernel on an n-qubit register"""
    return -(-(1 << n) // (reduce_blocks(1 << n) * REDUCE_THREADS))


def deflation_launches(B, J):
    """ovqe_deflation_info [5] on path 2: per row and pass one k_deflate_dots, one k_reduce per vector, one k_deflate_axpy"""
    return B * (2 * -(-J // DEFLATE_CHUNK) + J)


# ---- the cover rule, restated ------------------------------------------------------------------------------------------------------------
def _popcount(v):
    return bin(int(v)).count("1")


def grow_tile_set(masks, seed, M, n_bits):
    """grow_tile_set of csrc/sv_cover_host.hpp: from the seed bits the set grows, up to M bits, by the bit that brings the most masks
    within reach (a mask with nm missing bits scores 4^-(nm - 1) on each of them; equal scores: the lowest bit) until no mask that still
    fits is outside, then it is filled up with the lowest free bits"""
    S = int(seed)
    while _popcount(S) < M:
        room = M - _popcount(S)
        score = [0.0] * 64
        found = False
        for x in masks:
            miss = int(x) & ~S
            nm = _popcount(miss)
            if nm == 0 or nm > room:
                continue
            found = True
            for b in range(64):
                if (miss >> b) & 1:
                    score[b] += 0.25 ** min(nm - 1, 7)
        if not found:
            break
        best = -1
        for b in range(n_bits):
            if not (S >> b) & 1 and (best < 0 or score[b] > score[best]):
                best = b
        S |= 1 << best
    b = 0
    while _popcount(S) < M:
        S |= 1 << b
        b += 1
    return S


def apply_cover(n, hx, M=TILE_BITS, low=TILE_LOW):
    """the cover build_ham_tiles gives the x-groups of a Hamiltonian on a complex n-qubit register -> (bit sets of the sweeps, groups left
    untiled); ([], all groups): the register or the Hamiltonian is not tiled at all (tile_ok: n >= M + 2; at least three x-groups)"""
    groups = sorted({int(x) for x in hx})
    if n < M + 2 or len(groups) < 3:
        return [], len(groups)
    lowbits = (1 << low) - 1
    left = [x for x in groups if _popcount(x | lowbits) <= M]
    rest = len(groups) - len(left)
    sweeps = []
    while left:
        S = grow_tile_set(left, lowbits, M, n)
        assert any(not x & ~S for x in left)
        left = [x for x in left if x & ~S]
        sweeps.append(S)
    return sweeps, rest


def tiled_by_default(n):
    """whether apply_hamiltonian takes k_tile_apply under the default "apply_min_tiles" (the cover permitting)"""
    return (1 << n) >> TILE_BITS >= APPLY_MIN_TILES


# ---- cases -------------------------------------------------------------------------------------------------------------------------------
def explicit_case(n, hf, rx, rz, rc, pidx, K, hx, hz, hc, constant, phi0=None):
    """a ``gradbatch_cases.Case`` of a rotation program with THIS Hamiltonian (index-bit masks, real coefficients), term for term"""
    hx, hz, hc = np.asarray(hx, np.uint64), np.asarray(hz, np.uint64), np.asarray(hc, np.float64)
    case = gc.Case(n, hf, rx, rz, rc, pidx, K, phi0=phi0, ham=hessian_cases.hamiltonian_object(n, hx, hz, hc, constant))
    case.h = (hx, hz, hc, float(constant))
    case.h1 = hessian_cases.norm1(hc, constant)
    return case


BOUNDARY_C = 0.45           # the coefficient of Z on index bit 16, the term the 17-qubit Hamiltonian has beyond the 16-qubit one
BOUNDARY_LEAK = 0.3         # X on index bit 9: outside the support (index bits 0 to 6), as ``spread_cases.leak_case``


def boundary_pair(leak=True):
    """one real rotation program on the low index bits on both sides of COMPACT_MAX_QUBITS -> (case at 16 qubits, case at 17 qubits).
    The program is ``gradbatch_cases.per_rotation(9)``'s: Y rotations round index bits 0 to 6 from |0...0>, m = 128, K = 9; its masks are
    index-bit masks, so the same arrays are the same program on every register that holds them.  The Hamiltonian at 16: 20 random real
    terms whose x masks come from the program's (the support is closed under them) and whose z masks run over all 16 bits, one of them
    forced onto index bit 15.  At 17: the same terms, term for term, and BOUNDARY_C Z on index bit 16, which stays |0>: E17 = E16 +
    BOUNDARY_C, equal gradients.  ``leak``: both carry BOUNDARY_LEAK X on index bit 9 as well — <H> does not see it, ||H psi||^2 does, and
    the spread call streams on both registers (reasons 3 and 1); without it the spread call is on its path 1 at 16"""
    base = gc.per_rotation(9)
    n = COMPACT_MAX_QUBITS
    hx, hz, hc = hessian_cases.random_real_hamiltonian(n, 20, 1617, x_pool=base.rx)
    hz = hz.copy()
    hz[1] |= np.uint64(1 << (n - 1))                                               # the Z-only term reaches the top bit of the 16-qubit register
    if leak:
        hx, hz, hc = np.append(hx, np.uint64(1 << 9)), np.append(hz, np.uint64(0)), np.append(hc, BOUNDARY_LEAK)
    pair = []
    for nq in (n, n + 1):
        if nq > n:
            hx, hz, hc = np.append(hx, np.uint64(0)), np.append(hz, np.uint64(1 << n)), np.append(hc, BOUNDARY_C)
        pair.append(explicit_case(nq, 0, base.rx, base.rz, base.rc, base.pidx, base.K, hx, hz, hc, 0.25))
    return tuple(pair)


def complex_program(n, R):
    """R rotations round the index bits, rotation r on bit b = r mod n, parameter r mod ``gradbatch_cases.Y_K``: r mod 4 = 0: Y_b (odd Y:
    real); 1: X_b Z_(b+3) (no Y: a complex rotation); 2: Y_b Y_(b+1) (even Y); 3: Z_b Z_top (diagonal).  Every bit is in some x mask, the
    state fills the register with 16-byte amplitudes, no rotation-only real form exists, consecutive rotations differ in x.  From 12
    qubits on rotation 10 is Y_10 Y_11: its pairs straddle the edge of a 2^11 tile"""
    rx, rz = [], []
    for r in range(R):
        b, top = r % n, n - 1
        x, z = {0: (1 << b, 1 << b), 1: (1 << b, 1 << ((b + 3) % n)), 2: ((1 << b) | (1 << ((b + 1) % n)),) * 2,
                3: (0, (1 << b) | (1 << top))}[r % 4]
        rx.append(x)
        rz.append(z)
    rc = np.random.default_rng(4096 + n).uniform(0.5, 1.0, R)
    pidx = np.array([r % gc.Y_K for r in range(R)], np.int32)
    return np.array(rx, np.uint64), np.array(rz, np.uint64), rc, pidx


def is_real_program(rx, rz):
    """every rotation string has an odd number of Y: exp(-i phi P) is a real matrix"""
    return all(_popcount(int(x) & int(z)) % 2 == 1 for x, z in zip(rx, rz))


def _dense_hamiltonian(n, rx):
    """20 random real terms from the program's x masks (``hessian_cases.random_real_hamiltonian``): the first seed from 700 + n on whose
    cover at tiles of 2^TILE_BITS has at least two sweeps and no untiled rest"""
    for seed in range(700 + n, 764 + n):
        hx, hz, hc = hessian_cases.random_real_hamiltonian(n, 20, seed, x_pool=rx)
        sweeps, rest = apply_cover(n, hx)
        if len(sweeps) >= 2 and rest == 0 and 16 <= len(hc) <= 24:
            return hx, hz, hc
    raise AssertionError(f"no Hamiltonian with two tile sweeps at {n} qubits")


_DENSE = {}


def dense(n, real):
    """a program that fills an n-qubit register, n + 4 rotations, K = 24 -> ``gradbatch_cases.Case`` (cached: the checker's answers are
    kept on it).  ``real``: the rotations of ``gradbatch_cases.y_program(n + 4, n=n)``; else ``complex_program``.  The Hamiltonian:
    ``_dense_hamiltonian`` — x masks single bits of the register and pairs of them, so the sweeps of its cover are few and more than one"""
    key = (int(n), bool(real))
    if key not in _DENSE:
        if real:
            base = gc.y_program(n + 4, n=n)
            rx, rz, rc, pidx = base.rx, base.rz, base.rc, base.pidx
        else:
            rx, rz, rc, pidx = complex_program(n, n + 4)
        hx, hz, hc = _dense_hamiltonian(n, rx)
        _DENSE[key] = explicit_case(n, 0, rx, rz, rc, pidx, gc.Y_K, hx, hz, hc, 0.25)
    return _DENSE[key]


def thetas(case, B, seed):
    return np.random.default_rng(seed).uniform(-0.7, 0.7, (B, case.K))


# ---- deflation vectors -------------------------------------------------------------------------------------------------------------------
def vector_set(case, J, ncomplex=1, seed=50):
    """J vectors with distinct weights for ``case``'s register -> [(kind, vector or theta, beta)]: ``ncomplex`` complex
    ``deflation_cases.random_vector``, then — where at least two more are wanted — one real one, then "ansatz" states (theta:
    ``deflation_cases.case_state`` gives the vector).  J = 1: a complex vector; 2: it and an ansatz state; 4, 5: a complex and a real
    vector and two, three ansatz states; J = 32 with ``ncomplex`` = 30: thirty complex vectors, a real one, an ansatz state"""
    assert 1 <= J <= DEFLATE_MAX and 0 <= ncomplex <= J
    out = []
    rng = np.random.default_rng(seed + J)
    for j in range(J):
        beta = 0.5 + 0.125 * j
        if j < ncomplex:
            out.append(("vector", dc.random_vector(case.n, seed + 40 * J + j), beta))
        elif j == ncomplex and J - ncomplex >= 2:
            out.append(("vector", dc.random_vector(case.n, seed + 40 * J + j, real=True), beta))
        else:
            out.append(("ansatz", rng.uniform(-0.7, 0.7, case.K), beta))
    return out


def nested_set(case, seed=90):
    """DEFLATE_MAX entries whose prefixes are the sets of the vector-count test: a complex vector (J = 1), a real one, an ansatz state,
    a complex vector (J = 4: one full pass), another (J = 5: a pass and a remainder of one), and complex vectors up to J = 32 — thirty
    complex vectors, a real one and an ansatz state, distinct weights"""
    rng = np.random.default_rng(seed)
    out = []
    for j in range(DEFLATE_MAX):
        beta = 0.25 + 0.0625 * j
        if j == 2:
            out.append(("ansatz", rng.uniform(-0.7, 0.7, case.K), beta))
        else:
            out.append(("vector", dc.random_vector(case.n, seed + j, real=(j == 1)), beta))
    return out


def set_vectors(case, vset):
    """the vectors of a ``vector_set`` on the CPU"""
    return [dc.case_state(case, v) if kind == "ansatz" else v for kind, v, _ in vset]


def real_rows(vectors, support=None):
    """ovqe_deflation_info [4] on path 1: a row for Re phi_j, and one for Im phi_j where it is non-zero anywhere on the support"""
    sel = slice(None) if support is None else np.asarray(support, np.int64)
    return sum(1 + int(np.any(np.asarray(v)[sel].imag != 0.0)) for v in vectors)
