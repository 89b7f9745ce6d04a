"""TEST INFRASTRUCTURE ONLY — rotation lists that reach the table caps of the LDS-tiled rotation kernels, a restatement of the
planner's cut, and references that scale to shards of 21 and 25 local qubits.

``ovqe_apply_pauli_rotations`` (k_tile_sweep) and ``ovqe_adjoint_rotations`` (k_tile_adjoint, k_adjoint_pairs / k_adjoint_diag) cut a
list into same-x runs ("ops") and the ops into tile segments with ``build_tile_plan`` (openvqe_amd/csrc/tile_host.inc).  A forward
segment stages at most TILE_ROT_CAP = 256 table entries, a backward one 128 (tiles of 2^11) or 256 (2^12), and a streamed run goes
backwards in chunks of ADJ_MAX_ROT = 16.  ``plan`` is that cut in Python, the builders below make lists whose cut lands on each side of
the caps, and the GPU tests (tests/test_gpu_rotation_caps.py) compare the product's pass counters with the model — an accidental change
of 256 / 128 / 16, or of the greedy rule, shows there."""
from collections import namedtuple

import numpy as np

from oracle import masks

TILE_ROT_CAP = 256
ADJ_MAX_ROT = 16


def adjoint_rot_cap(M):
    """tile_adj_rot_cap (csrc/sv_tile.hpp)"""
    return TILE_ROT_CAP if M >= 12 else TILE_ROT_CAP // 2


def popcount(v):
    return bin(int(v)).count("1")


def same_x_runs(xs):
    """-> [(x, first, count)]: the ops of a list"""
    ops, a = [], 0
    while a < len(xs):
        b = a + 1
        while b < len(xs) and xs[b] == xs[a]:
            b += 1
        ops.append((int(xs[a]), a, b - a))
        a = b
    return ops


# kind "seg": ops [op0, op1) in one tile sweep on the index bits ``tile`` (a mask of M bits), rotations [rot0, rot0 + nrot);
# kind "op": op op0 on a sweep of its own (``tile`` = 0)
Step = namedtuple("Step", "kind op0 op1 rot0 nrot tile")


class Plan:
    def __init__(self, ops, steps):
        self.ops, self.steps = ops, steps
        self.segments = [s for s in steps if s.kind == "seg"]
        self.streamed = [s.op0 for s in steps if s.kind == "op"]
        self.forward_passes = len(steps)
        self.backward_passes = len(self.segments) + sum(-(-self.ops[i][2] // ADJ_MAX_ROT) for i in self.streamed)


def plan(xs, n_local, M, cap, low=4):
    """The greedy cut of build_tile_plan for tiles of 2^M amplitudes and ``cap`` table entries (under "real_state" M is tile_bits + 1
    and the rule is the same).  Nothing is tiled below two ops or when n_local < M + 2.  From S = the ``low`` lowest bits, ops are taken
    while |S u x| <= M and the rotations taken stay within cap (x = 0 needs no bits); fewer than two taken: the op keeps its own sweep."""
    ops = same_x_runs(xs)
    if len(ops) < 2 or n_local < M + 2:
        return Plan(ops, [Step("op", i, i + 1, ops[i][1], ops[i][2], 0) for i in range(len(ops))])
    steps, i = [], 0
    while i < len(ops):
        S, j, nrot = (1 << low) - 1, i, 0
        while j < len(ops):
            x, _, count = ops[j]
            if popcount(S | x) > M or nrot + count > cap:
                break
            S |= x
            nrot += count
            j += 1
        if j - i < 2:
            steps.append(Step("op", i, i + 1, ops[i][1], ops[i][2], 0))
            i += 1
            continue
        b = 0
        while popcount(S) < M:        # filled with the lowest free bits
            S |= 1 << b
            b += 1
        steps.append(Step("seg", i, j, ops[i][1], nrot, S))
        i = j
    return Plan(ops, steps)


# ---- list builders ---------------------------------------------------------------------------------------------------------------
PLACEMENTS = ("low", "high")


def bank(M, n_local, placement):
    """the M - 4 index bits (beside bits 0..3) a list's x masks live on, so that all its ops fit ONE tile: "low" = bits 4..M-1 (a
    contiguous tile), "high" = bits 4..M-2 and the top local bit (the tiles are not contiguous, TileSeg::mask_hi carries a far bit)"""
    if placement == "low":
        return sum(1 << b for b in range(4, M))
    if placement == "high":
        return sum(1 << b for b in range(4, M - 1)) | (1 << (n_local - 1))
    raise ValueError(placement)


def sign_bit(tile, n_local):
    """the highest local bit outside the tile: the one that differs between the tiles t and t + ntiles / 2 of one segment"""
    return max(b for b in range(n_local) if not (tile >> b) & 1)


def make_list(rng, pieces, n_local, g=0, real=False):
    """pieces: [(bank mask, [run length or (run length, "diag" | "full" | "wide12")])] -> xs, zs, phis (python ints / floats).
    Every run's x is a random non-empty subset of its bank and of bits 0..3, different from its neighbours'; "full" runs carry the
    whole bank (the first run of every piece does: the segment's tile is then bits 0..3 + the bank whatever else is drawn), "diag"
    runs have x = 0, "wide12" ones 12 bits above bit 3 (no tile holds them).  z is random over all n_local + g bits — bits outside
    the tile and rank bits give per-tile and per-shard signs — and the first rotation of every run has z on ``sign_bit``.  real: z is
    adjusted so that every string has an odd number of Y."""
    n = n_local + g
    xs, zs, phis = [], [], []
    prev = None
    for bk, runs in pieces:
        tile = bk | 15
        for k, item in enumerate(runs):
            count, tag = item if isinstance(item, tuple) else (item, "full" if k == 0 else "")
            while True:
                if tag == "diag":
                    x = 0
                elif tag == "wide12":
                    x = sum(1 << int(b) for b in rng.choice(np.arange(4, n_local), 12, replace=False))
                else:
                    x = int(rng.integers(0, 1 << n_local)) & tile
                    if tag == "full":
                        x |= bk
                if x != prev and (x or tag == "diag"):
                    break
            prev = x
            for r in range(count):
                z = int(rng.integers(0, 1 << n))
                if r == 0 and tag != "wide12":
                    z |= 1 << sign_bit(tile, n_local)
                if real and not popcount(x & z) & 1:
                    z ^= x & -x
                xs.append(x)
                zs.append(z)
                phis.append(float(rng.uniform(-1, 1)))
    return xs, zs, phis


# name -> run lengths as a function of the cap C (distinct x between neighbours); the cut each one must get is stated with the
# builders' CPU test (tests/test_rotation_cases.py) and in expected_cut below
BUILDERS = {
    "exact": lambda C: [C - 40, 24, 16],                         # one segment of exactly C rotations
    "exact_diag": lambda C: [C - 30, (20, "diag"), 10],          # ... with an OP_DIAG inside (complex amplitudes only)
    "one_over": lambda C: [C - 40, 24, 16, 1],                   # full segment, the last op on its own sweep
    "two_segments": lambda C: [C - 40, 24, (17, "full"), 5, 3],  # the cap closes a segment of C - 16; the second has rot0 = C - 16
    "long_run": lambda C: [3, C + 1, (3, "full"), 2],            # op 0 and the run of C + 1 streamed (last backward chunk: one
                                                                 # rotation), then one segment
    "run_of_cap": lambda C: [C, (2, "full"), 2],                 # the run of C streamed in exactly C / 16 chunks, then one segment
}
COMPLEX_BUILDERS = tuple(BUILDERS)
REAL_BUILDERS = tuple(b for b in BUILDERS if b != "exact_diag")


def expected_cut(name, C):
    """-> (segments as (first op, ops, rot0, rotations), streamed ops) the planner must give for a builder's list"""
    return {
        "exact": ([(0, 3, 0, C)], []),
        "exact_diag": ([(0, 3, 0, C)], []),
        "one_over": ([(0, 3, 0, C)], [3]),
        "two_segments": ([(0, 2, 0, C - 16), (2, 3, C - 16, 25)], []),
        "long_run": ([(2, 2, C + 4, 5)], [0, 1]),
        "run_of_cap": ([(1, 2, C, 4)], [0]),
    }[name]


def build(name, C, M, n_local, g=0, placement="low", real=False, seed=0):
    """the list of builder ``name`` for table cap C and tiles of 2^M amplitudes"""
    tag = sum(ord(c) for c in name + placement)
    rng = np.random.default_rng([seed, tag, C, M, n_local, g, int(real)])
    return make_list(rng, [(bank(M, n_local, placement), BUILDERS[name](C))], n_local, g, real)


def multi_tile_list(M, n_local, g=0, seed=0):
    """Three segments separated by bank changes — runs 5, 4 on the low bank / 3, 1, 2 on the high bank / a wide op / 6, 2 on a third
    bank (bits M .. 2M - 5) — for shards on which one workgroup of k_tile_adjoint walks several tiles."""
    rng = np.random.default_rng([seed, 77, M, n_local, g])
    third = sum(1 << b for b in range(M, 2 * M - 4))
    return make_list(rng, [(bank(M, n_local, "low"), [5, 4]), (bank(M, n_local, "high"), [3, 1, 2, (1, "wide12")]),
                           (third, [6, 2])], n_local, g)


def production_forward_list(real, seed=0, n_local=25):
    """about 24 rotations for the 25-qubit forward sweeps: a segment on bank bits 4..9, a wide op on both banks, a segment on bank
    bits 19..24; of bits 0..3 only 0 and 2 are used, so the union of the x masks has 14 bits (fibre_reference)"""
    rng = np.random.default_rng([seed, 2525, int(real)])
    A, B, low = sum(1 << b for b in range(4, 10)), sum(1 << b for b in range(n_local - 6, n_local)), 0b0101
    xs, zs, phis = [], [], []
    prev = None
    for bk, runs in ((A, [4, 3, 4]), (A | B, [2]), (B, [3, 4, 4])):
        for k, count in enumerate(runs):
            while True:
                x = (int(rng.integers(0, 1 << n_local)) & (bk | low)) | (bk if k == 0 else 0)
                if x and x != prev:
                    break
            prev = x
            for r in range(count):
                z = int(rng.integers(0, 1 << n_local))
                if r == 0:
                    z |= 1 << (n_local - 1 if bk == A else 12)      # a bit outside the segment's tile (bits 0..12 at most / B's)
                if real and not popcount(x & z) & 1:
                    z ^= x & -x
                xs.append(x)
                zs.append(z)
                phis.append(float(rng.uniform(-1, 1)))
    return xs, zs, phis


def production_backward_list(seed=0, n_local=25):
    """six rotations, two segments for tiles of 2^12: runs 2, 1 on bank bits 4..11, then 1, 2 on bits 17..24"""
    rng = np.random.default_rng([seed, 2526])
    A, B = sum(1 << b for b in range(4, 12)), sum(1 << b for b in range(n_local - 8, n_local))
    return make_list(rng, [(A, [2, 1]), (B, [1, 2])], n_local, 0)


# ---- references ------------------------------------------------------------------------------------------------------------------
def adjoint_reference_c(psi, lam, xs, zs, phis, nl, g):
    """The contract of ``_reference`` in tests/test_gpu_shard_gradient.py — per shard the sums w[s, r] = Im <lam_s|P_r|psi_s>, both
    vectors un-rotated last to first -> w[2^g, R], psi, lam before the list — on the plain-C oracle (OpenMP; numpy needs 0.4 s per
    rotation at 2^21 amplitudes): per rotation, last to first, tmp = exp(-i pi/2 P) psi = -i P psi (up to cos(pi/2) = 6e-17 of psi), so Im <lam|P|psi> = Re <lam|tmp>; then psi and lam
    are rotated by -phi.  x masks are local, so the rotation of the whole register is the rotation of every shard with its rank-bit
    signs."""
    from oracle import cref
    L = cref.lib()
    n = nl + g
    psi, lam = np.ascontiguousarray(psi, np.complex128).copy(), np.ascontiguousarray(lam, np.complex128).copy()
    w = np.zeros((1 << g, len(xs)))
    tmp = np.empty_like(psi)
    for r in range(len(xs) - 1, -1, -1):
        x, z, p = int(xs[r]), int(zs[r]), float(phis[r])
        np.copyto(tmp, psi)
        L.orc_pauli_rotation(tmp, n, x, z, np.pi / 2)
        for s in range(1 << g):
            sl = slice(s << nl, (s + 1) << nl)
            w[s, r] = np.vdot(lam[sl], tmp[sl]).real
        L.orc_pauli_rotation(psi, n, x, z, -p)
        L.orc_pauli_rotation(lam, n, x, z, -p)
    return w, psi, lam


def _deposit(e, mask):
    out = np.zeros_like(e)
    k = 0
    for b in range(64):
        if (mask >> b) & 1:
            out |= ((e >> np.uint64(k)) & np.uint64(1)) << np.uint64(b)
            k += 1
    return out


def _extract(v, mask):
    out, k = 0, 0
    for b in range(64):
        if (mask >> b) & 1:
            out |= ((v >> b) & 1) << k
            k += 1
    return out


def fibre_reference(seed, scale, i, xs, zs, phis, real=False):
    """A list whose x masks have union U only mixes amplitudes inside a fibre {(i & ~U) | deposit(e, U)}: the inputs on the fibre of
    index i come from the synthetic state's formula (openvqe_amd/synth.py; their real parts under ``real``), the rotations are applied
    on that vector of 2^|U| amplitudes with the signs read off the GLOBAL indices, (P a)_i = i^ny (-1)^|(i ^ x) & z| a_(i ^ x).
    -> (global indices of the fibre, expected amplitudes) — no host copy of the state"""
    from openvqe_amd import synth
    U = 0
    for x in xs:
        U |= int(x)
    k = popcount(U)
    if k > 14:
        raise ValueError("the union of the x masks has more than 14 bits")
    e = np.arange(1 << k, dtype=np.uint64)
    G = _deposit(e, U) | np.uint64(int(i) & ~U)
    a = synth.amplitudes(seed, G) * scale
    if real:
        a = a.real.astype(np.complex128)
    ei = e.astype(np.int64)
    for x, z, p in zip(xs, zs, phis):
        x, z = int(x), int(z)
        sign = 1.0 - 2.0 * masks._parity((G ^ np.uint64(x)) & np.uint64(z))
        pa = (1j) ** (popcount(x & z) % 4) * sign * a[ei ^ _extract(x, U)]
        a = np.cos(p) * a - 1j * np.sin(p) * pa
    return G, a
