"""Pools for the tests of the planned ADAPT screen on the partitioned register (ovqe_xpool_*, ShardedStatevector.pool_gradients):
the shapes the planner of openvqe_amd/csrc/sv_pool_host.hpp has a path of its own for, and the term-by-term oracle."""
import numpy as np

from oracle import masks


def edge_pool(rng, n, n_local, big=True):
    """[(xs, zs, coeffs) per operator] on n qubits: random operators of 1..3 strings with x anywhere in the register; two operators
    sharing one x mask; an operator spread over several partners and several passes (x on the rank bits, on the bits above any
    chunk, on the low bits); a diagonal operator; an operator with no terms; with ``big`` an operator with more terms on one x than
    TILE_TERM_CAP (512) and more (operator, x) entries inside one pass than the group cap (150 single-string operators whose x
    masks lie on the four lowest bits)"""
    dim = 1 << n

    def z():
        return int(rng.integers(0, dim))

    pool = []
    for _ in range(6):
        nt = int(rng.integers(1, 4))
        pool.append(([int(rng.integers(0, dim)) for _ in range(nt)], [z() for _ in range(nt)],
                     list(rng.normal(size=nt) + 1j * rng.normal(size=nt))))
    shared = int(rng.integers(0, 32)) | (1 << (n - 1))
    pool.append(([shared], [z()], [1.0 + 0.5j]))
    pool.append(([shared, shared], [z(), z()], [-0.25 + 0j, 2.0j]))
    spread = [int(rng.integers(0, dim)) for _ in range(6)] + [dim - 1, 1 << (n - 1), 1 << (n_local - 1), 3]
    pool.append((spread, [z() for _ in spread], list(rng.normal(size=len(spread)) + 1j * rng.normal(size=len(spread)))))
    pool.append(([0, 0], [z() | 1, z()], [0.7 + 0j, -0.2j]))
    pool.append(([], [], []))
    if big:
        xb = 5 | ((1 << n_local) if n > n_local else 0)
        pool.append(([xb] * 530, [z() for _ in range(530)], list((rng.normal(size=530) + 1j * rng.normal(size=530)) / 530.0)))
        for _ in range(150):
            pool.append(([int(rng.integers(0, 16))], [z()], [complex(rng.normal())]))
    return pool


def flatten(pool):
    """-> CSR offsets, xs, zs, coeffs"""
    offsets = np.zeros(len(pool) + 1, np.int64)
    np.cumsum([len(op[0]) for op in pool], out=offsets[1:])
    xs = np.array([int(x) for op in pool for x in op[0]], np.uint64)
    zs = np.array([int(z) for op in pool for z in op[1]], np.uint64)
    cs = np.array([complex(c) for op in pool for c in op[2]], np.complex128)
    return offsets, xs, zs, cs


def bilinear_oracle(pool, sigma, psi):
    """v_k = sum_t c_t <sigma|P_t|psi> and |c_k|_1 per operator, term by term on the whole register"""
    v = np.array([sum((c * np.vdot(sigma, masks.pauli_apply(psi, int(x), int(z))) for x, z, c in zip(*op)), 0j) for op in pool])
    l1 = np.array([max(1.0, float(np.abs(np.asarray(op[2], complex)).sum())) if len(op[2]) else 1.0 for op in pool])
    return v, l1
