"""Pauli sums for the tests of the tile-cover kernels at their staging caps (tests/test_gpu_cover_caps.py): a staged chunk of the cover
holds at most TILE_TERM_CAP = 512 terms and TILE_APPLY_GROUPS = 128 pieces (openvqe_amd/csrc/sv_cover_host.hpp), a group with more terms
is cut into pieces, a pass or sweep with more pieces restages its tables.  The builders are seeded and return (xs, zs, cs) as
np.uint64 / np.uint64 / np.complex128 in the physical index-bit space of a register of n = n_local + g qubits; the states and the
term-by-term references that the GPU tests compare with are made once per sum (``reference``) and handed out read-only."""
import functools

import numpy as np

from oracle import masks

TERM_CAP = 512     # TILE_TERM_CAP
GROUP_CAP = 128    # TILE_APPLY_GROUPS
STYLES = ("symmetric", "hermitian", "complex")
IDENT = 0.3        # sigma = (H + IDENT) psi


def popcount(v):
    return bin(int(v)).count("1")


def odd_y(xs, zs):
    return np.array([popcount(int(x) & int(z)) & 1 for x, z in zip(xs, zs)], bool)


def _styled(rng, xs, zs, style):
    """the coefficient class of a sum: "symmetric" = real coefficients and an even number of Y in every string (a Y is moved off the
    lowest x bit where the count is odd: z & ~x stays), "hermitian" = real coefficients, z as drawn (about half the strings carry an
    odd number of Y: the folded coefficient c i^ny is imaginary), "complex" = coefficients a + ib.  N(0, 1), not scaled down: a
    dropped or doubled term moves a result by far more than any bound in use"""
    xs = np.array([int(x) for x in xs], np.uint64)
    zs = np.array([int(z) for z in zs], np.uint64)
    if style == "symmetric":
        zs = np.where(odd_y(xs, zs), zs ^ (xs & (~xs + np.uint64(1))), zs)
    elif style not in STYLES:
        raise ValueError(style)
    cs = rng.normal(size=len(xs)).astype(np.complex128)
    if style == "complex":
        cs = cs + 1j * rng.normal(size=len(xs))
    return xs, zs, cs


def _distinct(rng, below, count, exclude=()):
    pool = np.array([v for v in range(below) if v not in exclude])
    return [int(v) for v in rng.choice(pool, count, replace=False)]


def _deposit(v, hole_mask, n):
    """the bits of v spread over the positions of an n-bit word outside hole_mask, ascending"""
    out, k = 0, 0
    for b in range(n):
        if not (hole_mask >> b) & 1:
            out |= ((v >> k) & 1) << b
            k += 1
    return out


def _inside_shard(rng, n, low_groups=230):
    """the d = 0 strings: a diagonal group of 600 strings with pairwise distinct z; one group at x = 0b101 of 530 strings whose z & ~x are
    pairwise distinct (no merging of terms that agree outside x can bring it under 512, whatever the tile set); ``low_groups``
    single-term groups on distinct masks below 2^8 (neither 0 nor 0b101; there are 254 of those: above 230 groups the masks are
    drawn below 2^9)"""
    dim = 1 << n
    xs = [0] * 600
    zs = _distinct(rng, dim, 600)
    xs += [0b101] * 530
    zs += [_deposit(w, 0b101, n) | (int(rng.integers(0, 2)) | int(rng.integers(0, 2)) << 2) for w in _distinct(rng, dim >> 2, 530)]
    xs += _distinct(rng, 1 << (8 if low_groups <= 230 else 9), low_groups, exclude=(0, 0b101))
    zs += [int(v) for v in rng.integers(0, dim, low_groups)]
    return xs, zs


def staging_sum(rng, n, n_local, style):
    """for every non-zero rank difference d: 200 single-term groups whose local x masks are distinct values below 2^8, the same 200
    masks with local bit n_local - 1 as well (above every chunk smaller than the shard: a second class of x bits above the chunk) and
    530 more terms on the first of those masks (a group of 531 terms: cut); inside the shard the strings of ``_inside_shard``"""
    dim = 1 << n
    xs, zs = [], []
    for d in range(1, 1 << (n - n_local)):
        low = _distinct(rng, 1 << 8, 200)
        xs += [(d << n_local) | m for m in low]
        xs += [(d << n_local) | m | (1 << (n_local - 1)) for m in low]
        xs += [(d << n_local) | low[0]] * 530
        zs += [int(v) for v in rng.integers(0, dim, 930)]
    lx, lz = _inside_shard(rng, n)
    return _styled(rng, xs + lx, zs + lz, style)


def geometry_sum(rng, n, n_local, style):
    """80 strings with x anywhere in the register — rank bits, bits above every chunk, low bits — and a few repeated masks: many
    passes of few groups each, with the coefficient classes of ``staging_sum``"""
    dim, g = 1 << n, n - n_local
    T = 80
    xs = [int(v) for v in rng.integers(0, dim, T)]
    xs[:6] = [0] * 6                                                  # a diagonal group
    xs[6:14] = [x & ((1 << n_local) - 1) for x in xs[6:14]]           # groups inside the shard
    xs[14:18] = [xs[14]] * 4                                          # a group of four terms
    xs[18] = 1 << (n - 1)                                             # one rank bit alone
    xs[19] = ((1 << g) - 1) << n_local                                # every rank bit
    xs[20] = (1 << n_local) | 1 | (1 << (n_local - 1))                # lowest rank bit, top and bottom local bit
    xs[21:24] = [xs[20]] * 3
    xs[24:27] = [xs[18] | 0b110] * 3
    zs = [int(v) for v in rng.integers(0, dim, T)]
    return _styled(rng, xs, zs, style)


def register_sum(rng, n, style, low_groups=230):
    """one register (g = 0): the inside-the-shard half of ``staging_sum``, the low-mask family cut to ``low_groups`` groups, and 20
    strings with z as drawn (odd numbers of Y among them) on masks below 2^8.  popcount(x | 3) <= 10 for every x: no group is left
    outside a tile of 2^10 amplitudes or more"""
    lx, lz = _inside_shard(rng, n, low_groups)
    xs, zs, cs = _styled(rng, lx, lz, style)
    ex = np.array([int(v) for v in rng.integers(1, 1 << 8, 20)], np.uint64)
    ez = np.array([int(v) for v in rng.integers(0, 1 << n, 20)], np.uint64)
    return np.concatenate([xs, ex]), np.concatenate([zs, ez]), np.concatenate([cs, rng.normal(size=20).astype(np.complex128)])


BUILDERS = {"staging": staging_sum, "geometry": geometry_sum}


def distinct_local_x(xs, zs, n_local, even_y_only=False):
    """{rank difference d != 0: number of distinct local x masks}; ``even_y_only``: of the strings with an even number of Y (between
    real vectors the planner leaves the others out)"""
    keep = ~odd_y(xs, zs) if even_y_only else np.ones(len(xs), bool)
    out = {}
    for x in np.asarray(xs)[keep]:
        d = int(x) >> n_local
        if d:
            out.setdefault(d, set()).add(int(x) & ((1 << n_local) - 1))
    return {d: len(v) for d, v in out.items()}


def dense_state(rng, n, real=False):
    psi = rng.normal(size=1 << n) + (0.0 if real else 1j * rng.normal(size=1 << n))
    return (psi / np.linalg.norm(psi)).astype(np.complex128)


def one_per_shard_state(rng, n, n_local, xs, real=False):
    """normalised, ONE non-zero amplitude per shard (every other ket tile is a tile of zeros), placed so that a string of the sum connects
    shard 0's amplitude with every other shard's: position p0 in shard 0, p0 ^ (local x of the first string with rank difference s)
    in shard s"""
    W = 1 << (n - n_local)
    p0 = int(rng.integers(0, 1 << n_local))
    psi = np.zeros(1 << n, np.complex128)
    for s in range(W):
        xl = next((int(x) & ((1 << n_local) - 1) for x in xs if int(x) >> n_local == s), 0) if s else 0
        psi[(s << n_local) | (p0 ^ xl)] = (-1.0 if s & 1 else 1.0) if real else np.exp(1j * (0.7 + 1.1 * s))
    return psi / np.sqrt(W)


def sparse_state(rng, n, real=False, empty_block_bits=None):
    """normalised, one amplitude in eight non-zero at random positions (every tile is at most a quarter full: the sparse-tile path of
    k_tile_expect); ``empty_block_bits`` = b: every second aligned block of 2^b amplitudes emptied as well"""
    dim = 1 << n
    psi = np.zeros(dim, np.complex128)
    pos = rng.choice(dim, dim // 8, replace=False)
    psi[pos] = rng.normal(size=len(pos)) + (0.0 if real else 1j * rng.normal(size=len(pos)))
    if empty_block_bits is not None:
        psi[((np.arange(dim) >> empty_block_bits) & 1) == 1] = 0.0
    return psi / np.linalg.norm(psi)


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def reference(builder, n, n_local, style, real=False):
    """the sum ``builder`` (a key of BUILDERS) with its two states and their references from the bit-mask oracle applied on the whole
    register, separately to the strings inside the shards (rank difference 0) and across them: -> dict with xs, zs, cs, l1 = |c|_1 and
    states = [(name, psi, H_0 psi, H_cross psi)].  Computed once per key; the arrays are read-only"""
    rng = np.random.default_rng([n, n_local, STYLES.index(style), int(real), sorted(BUILDERS).index(builder)])
    xs, zs, cs = BUILDERS[builder](rng, n, n_local, style)
    inside = (xs >> np.uint64(n_local)) == 0
    states = []
    for name, psi in (("dense", dense_state(rng, n, real)), ("one_per_shard", one_per_shard_state(rng, n, n_local, xs, real))):
        h0 = masks.apply_pauli_sum(psi, xs[inside], zs[inside], cs[inside])
        hx = masks.apply_pauli_sum(psi, xs[~inside], zs[~inside], cs[~inside])
        states.append((name, _frozen(psi), _frozen(h0), _frozen(hx)))
    return {"xs": _frozen(xs), "zs": _frozen(zs), "cs": _frozen(cs), "l1": float(np.abs(cs).sum()), "states": states}
