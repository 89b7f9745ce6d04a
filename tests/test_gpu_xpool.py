"""The planned ADAPT pool screen of one shard, ovqe_xpool_* straight through the binding (csrc/pool_host.inc, kernels csrc/sv_pool.hpp):
several shard handles on one GPU stand for the ranks, there is no process group.  psi is random and sigma an independent random
vector; the sum over the ranks of v_k is compared with the bit-mask oracle on the whole register to 1e-11 max(1, |c_k|_1).

Shapes (n, rank bits, chunk bits).  The kernels instantiate tiles of 2^10 / 2^11 / 2^12 complex amplitudes and 2^11 / 2^12 / 2^13
doubles, chosen as min(largest, chunk bits); below 2^10 / 2^11 the streaming form runs.  Every tile size is met at its smallest
chunk with several chunks per shard, plus one case whose chunk is the whole shard."""
import numpy as np
import pytest

from oracle import masks
from tests.pool_cases import bilinear_oracle, edge_pool, flatten
from tests.util import random_state

pytestmark = pytest.mark.gpu

COMPLEX_SHAPES = [(12, 3, 7), (13, 2, 10), (15, 2, 11), (14, 1, 12), (13, 1, 12)]
REAL_SHAPES = [(12, 2, 8), (15, 2, 11), (16, 2, 12), (15, 1, 13)]


@pytest.fixture(scope="module")
def SV(gpu_lib):
    from openvqe_amd.backend import Statevector
    return Statevector


def _screen_once(shards, pids, bufs, bras, nl, chunk_bits, check_support=None):
    """enqueue every rank's local and remote contractions, then finish -> [v per rank]"""
    csize = 1 << chunk_bits
    out = []
    for s, (sv, pid) in enumerate(zip(shards, pids)):
        sv.xpool_local(pid, bras[s].data_ptr())
        for d, passes in sv.xpool_partners(pid):
            ket = bufs[s ^ d]
            for c in range(1 << (nl - chunk_bits)):
                sv.xpool_remote(pid, d, c, ket[c * csize:(c + 1) * csize].data_ptr(), bras[s].data_ptr())
                if check_support is not None:
                    assert sv.last_passes() == (passes, passes * check_support * csize)
        out.append(sv.xpool_finish(pid))
    return out


def _run_case(SV, n, g, chunk_bits, real, sparse_ket=False):
    import torch
    rng = np.random.default_rng(1000 * n + 10 * g + chunk_bits + (5 if real else 0))
    nl = n - g
    W = 1 << g
    pool = edge_pool(rng, n, nl)
    offsets, xs, zs, cs = flatten(pool)
    if sparse_ket:      # a basis state plus four rotations: zero outside a few tiles; sigma stays dense
        psi = np.zeros(1 << n, complex)
        psi[int(rng.integers(0, 1 << n))] = 1.0
        for _ in range(4):
            bits = [int(b) for b in rng.choice(n, 2, replace=False)]
            x = (1 << bits[0]) | (1 << bits[1])
            psi = masks.rotate(psi, x, (1 << bits[0]) if real else int(rng.integers(0, 1 << n)), float(rng.uniform(0.2, 1.0)))
        assert np.count_nonzero(psi) <= 16
    else:
        psi = random_state(rng, n)
    sigma = random_state(rng, n)
    if real:
        psi = psi.real / np.linalg.norm(psi.real) + 0j
        sigma = sigma.real / np.linalg.norm(sigma.real) + 0j
    want, l1 = bilinear_oracle(pool, sigma, psi)
    dt = torch.float64 if real else torch.complex128

    def dev(v, s):
        a = v[s << nl:(s + 1) << nl]
        return torch.from_numpy(np.ascontiguousarray(a.real if real else a)).to(dt).cuda()

    shards = [SV(nl, n_global=g, shard_index=s) for s in range(W)]
    bufs = [dev(psi, s) for s in range(W)]
    bras = [dev(sigma, s) for s in range(W)]
    try:
        pids = []
        for sv, b in zip(shards, bufs):
            sv.adopt_state(b.data_ptr())
            if real:
                sv.set_option("real_state", 1)
            pids.append(sv.xpool_create(offsets, xs, zs, cs, chunk_bits))
        info = shards[0].xpool_info(pids[0])
        streaming = chunk_bits < (11 if real else 10)
        assert info["operators"] == len(pool) and info["partial_bytes"] == 512 * len(pool) * 16
        assert info["partners"] == len(shards[0].xpool_partners(pids[0])) == len({int(x) >> nl for x in xs if int(x) >> nl})
        assert info["entries"] == len({(k, int(x)) for k, op in enumerate(pool) for x in op[0]}) >= info["x_masks"] > 0
        assert info["remote_passes_per_chunk"] <= info["x_masks"] and info["remote_passes_per_chunk"] == sum(p for _, p in shards[0].xpool_partners(pids[0]))
        if chunk_bits < nl:    # (a chunk that is the whole shard tiles both the remote and the local entries)
            assert info["streaming_fallback"] == (1 if streaming else 0)
        if not streaming:
            assert info["tile_bits"] == min(13 if real else 12, nl)    # (the d = 0 cover takes the shard as its chunk)
        first = _screen_once(shards, pids, bufs, bras, nl, chunk_bits, check_support=16 if real else 32)
        got = np.sum(first, axis=0)
        print("max |v - oracle| / max(1, |c|_1) = %.3e" % float((np.abs(got - want) / l1).max()))
        assert np.all(np.abs(got - want) <= 1e-11 * l1)
        # the accumulators were reset: a second finish returns exact zeros
        for sv, pid in zip(shards, pids):
            again = sv.xpool_finish(pid)
            assert np.all(again.real == 0.0) and np.all(again.imag == 0.0)
        # the reductions run in a fixed order: the same screen again gives the same bits
        second = _screen_once(shards, pids, bufs, bras, nl, chunk_bits)
        for a, b in zip(first, second):
            assert np.array_equal(a.view(np.float64), b.view(np.float64))
        return shards, pids, bufs, bras
    except BaseException:
        for sv in shards:
            sv.close()
        raise


@pytest.mark.parametrize("n,g,chunk_bits", COMPLEX_SHAPES)
def test_planned_pool_screen_complex_against_oracle(SV, n, g, chunk_bits):
    shards, *_ = _run_case(SV, n, g, chunk_bits, False)
    for sv in shards:
        sv.close()


@pytest.mark.parametrize("n,g,chunk_bits", REAL_SHAPES)
def test_planned_pool_screen_real_against_oracle(SV, n, g, chunk_bits):
    """option "real_state": bra and ket chunks are doubles, both parts of v_k are kept (imaginary folded coefficients give Im v_k)"""
    shards, *_ = _run_case(SV, n, g, chunk_bits, True)
    for sv in shards:
        sv.close()


@pytest.mark.parametrize("real", [False, True])
def test_planned_pool_screen_with_a_ket_on_a_few_tiles(SV, real):
    """a basis state plus four rotations as the ket (zero outside a few tiles: the all-zero tile early exit) and a dense sigma"""
    shards, *_ = _run_case(SV, 15, 2, 11, real, sparse_ket=True)
    for sv in shards:
        sv.close()


def test_planned_pool_refusals(SV):
    import torch
    from openvqe_amd._lib import BackendError
    n, g, chunk_bits = 13, 2, 10
    nl = n - g
    shards, pids, bufs, bras = _run_case(SV, n, g, chunk_bits, False)
    try:
        sv, pid = shards[0], pids[0]
        partners = [d for d, _ in sv.xpool_partners(pid)]
        one = np.array([1.0 + 0j])
        with pytest.raises(BackendError, match="chunk index beyond the shard"):
            sv.xpool_remote(pid, partners[0], 1 << (nl - chunk_bits), bufs[1].data_ptr(), bras[0].data_ptr())
        lone = sv.xpool_create([0, 1], [1 | (1 << nl)], [0], one, chunk_bits)       # entries for rank difference 1 only
        with pytest.raises(BackendError, match="no entries for this rank difference"):
            sv.xpool_remote(lone, 2, 0, bufs[2].data_ptr(), bras[0].data_ptr())
        with pytest.raises(BackendError, match="no entries for this rank difference"):
            sv.xpool_remote(lone, 0, 0, bufs[0].data_ptr(), bras[0].data_ptr())
        sv.xpool_destroy(lone)
        with pytest.raises(BackendError, match="bits beyond the register"):
            sv.xpool_create([0, 1], [1 << n], [0], one, chunk_bits)
        with pytest.raises(BackendError, match="offsets must start at 0 and never decrease"):
            sv.xpool_create([0, 2, 1], [1, 2], [0, 0], np.array([1.0 + 0j, 1.0]), chunk_bits)
        with pytest.raises(BackendError, match="chunk_bits"):
            sv.xpool_create([0, 1], [1], [0], one, nl + 1)
        with pytest.raises(BackendError, match="bra overlaps the state buffer"):
            sv.xpool_local(pid, bufs[0].data_ptr())
        with pytest.raises(BackendError, match="bra overlaps the state buffer"):
            sv.xpool_remote(pid, partners[0], 0, bufs[1].data_ptr(), bufs[0].data_ptr() + 16 * 8)
        # nothing was accumulated by the refused calls
        z = sv.xpool_finish(pid)
        assert np.all(z.real == 0.0) and np.all(z.imag == 0.0)
        sv.xpool_destroy(pid)
        with pytest.raises(BackendError, match="no such planned pool"):
            sv.xpool_local(pid, bras[0].data_ptr())
        with pytest.raises(BackendError, match="no such planned pool"):
            sv.xpool_finish(pid)
        torch.cuda.synchronize()
    finally:
        for s in shards:
            s.close()
