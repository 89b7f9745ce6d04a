"""CPU checks of tests/rotation_cases.py: the builders' lists get exactly the cut they are named after from the model of
build_tile_plan, every segment sees a per-tile sign, the real lists keep a real state real, and the two references of the large-shard
GPU tests (tests/test_gpu_rotation_caps.py) equal the numpy oracle where that one is fast enough."""
import numpy as np
import pytest

from oracle import masks
from tests import rotation_cases as rc
from tests.util import random_state

CUT_CASES = [(name, C, M, placement, real)
             for C in (128, 256) for M in (10, 11, 12, 13) for placement in rc.PLACEMENTS for real in (False, True)
             for name in (rc.REAL_BUILDERS if real else rc.COMPLEX_BUILDERS)
             if (11 <= M <= 13 if real else M <= 12)]      # tile sizes of the kernels: complex 2^10..2^12, real 2^11..2^13


@pytest.mark.parametrize("name,C,M,placement,real", CUT_CASES)
def test_builders_get_the_cut_they_are_named_after(name, C, M, placement, real):
    nl, g = M + 2, 1
    xs, zs, phis = rc.build(name, C, M, nl, g, placement, real)
    runs = [item[0] if isinstance(item, tuple) else item for item in rc.BUILDERS[name](C)]
    ops = rc.same_x_runs(xs)
    assert [count for _, _, count in ops] == runs                                  # distinct x between neighbours
    assert all(x >> nl == 0 for x in xs) and all(z >> (nl + g) == 0 for z in zs) and any(z >> nl for z in zs)
    p = rc.plan(xs, nl, M, C)
    segments, streamed = rc.expected_cut(name, C)
    assert [(s.op0, s.op1 - s.op0, s.rot0, s.nrot) for s in p.segments] == segments
    assert p.streamed == streamed
    assert p.forward_passes == len(segments) + len(streamed)
    assert p.backward_passes == len(segments) + sum(-(-runs[i] // 16) for i in streamed)
    tile = rc.bank(M, nl, placement) | 15
    for s in p.segments:
        assert s.tile == tile and rc.popcount(tile) == M
        assert any(z & ~tile & ((1 << nl) - 1) for z in zs[s.rot0:s.rot0 + s.nrot])     # a sign that differs between tiles
    assert (name == "exact_diag") == (0 in xs)
    if real:
        assert all(x and rc.popcount(x & z) & 1 for x, z in zip(xs, zs))            # odd number of Y, no diagonal string
    # what each list is for
    if name in ("exact", "exact_diag", "one_over"):
        assert p.segments[0].nrot == C
    if name == "two_segments":
        assert p.segments[0].nrot + runs[2] == C + 1 and p.segments[1].rot0 > 0
    if name == "long_run":
        assert runs[1] == C + 1 and runs[1] % 16 == 1 and p.backward_passes == 1 + (C // 16 + 1) + 1
    if name == "run_of_cap":
        assert p.backward_passes == C // 16 + 1


def test_model_leaves_small_shards_and_single_runs_untiled():
    xs, _, _ = rc.build("exact", 128, 11, 13)
    assert len(rc.plan(xs, 13, 11, 128).segments) == 1
    assert rc.plan(xs, 12, 11, 128).segments == [] and rc.plan(xs, 12, 11, 128).backward_passes == 6 + 2 + 1
    assert rc.plan([5] * 40, 14, 11, 128).segments == [] and rc.plan([5] * 40, 14, 11, 128).backward_passes == 3
    assert (rc.adjoint_rot_cap(11), rc.adjoint_rot_cap(12)) == (128, 256)


@pytest.mark.parametrize("M,nl,g", [(11, 21, 0), (12, 21, 0), (11, 21, 1)])
def test_multi_tile_list(M, nl, g):
    """three segments and a wide op; in every segment a rotation has z on the highest local bit outside the tile — the top local bit for
    the low banks, the one below it for the high bank, whose tile holds the top bit —: that bit is the one in which the tiles t and
    t + grid of one workgroup differ, so the sign of its sum differs between them"""
    xs, zs, phis = rc.multi_tile_list(M, nl, g)
    p = rc.plan(xs, nl, M, rc.adjoint_rot_cap(M))
    assert [count for _, _, count in p.ops] == [5, 4, 3, 1, 2, 1, 6, 2]
    assert [(s.op0, s.op1 - s.op0, s.rot0, s.nrot) for s in p.segments] == [(0, 2, 0, 9), (2, 3, 9, 6), (6, 2, 16, 8)]
    assert p.streamed == [5] and p.backward_passes == 4 and p.forward_passes == 4
    assert rc.popcount(xs[15]) == 12
    tops = []
    for s in p.segments:
        top = rc.sign_bit(s.tile, nl)
        tops.append(top)
        assert any((z >> top) & 1 for z in zs[s.rot0:s.rot0 + s.nrot])
    assert tops == [nl - 1, nl - 2, nl - 1]
    assert (p.segments[1].tile >> (nl - 1)) & 1
    if g:
        assert any(z >> nl for z in zs)


@pytest.mark.parametrize("real", [False, True])
def test_production_lists(real):
    xs, zs, phis = rc.production_forward_list(real)
    U = 0
    for x in xs:
        U |= x
    assert len(xs) == 24 and rc.popcount(U) == 14
    for M in ((13,) if real else (12,)):
        p = rc.plan(xs, 25, M, rc.TILE_ROT_CAP)
        assert [(s.op0, s.op1 - s.op0, s.rot0, s.nrot) for s in p.segments] == [(0, 3, 0, 11), (4, 3, 13, 11)] and p.streamed == [3]
        for s in p.segments:
            assert any(z & ~s.tile for z in zs[s.rot0:s.rot0 + s.nrot])
    if real:
        assert all(x and rc.popcount(x & z) & 1 for x, z in zip(xs, zs))
    else:
        xs, zs, phis = rc.production_backward_list()
        p = rc.plan(xs, 25, 12, rc.adjoint_rot_cap(12))
        assert [(s.op0, s.op1 - s.op0, s.rot0, s.nrot) for s in p.segments] == [(0, 2, 0, 3), (2, 2, 3, 3)] and p.backward_passes == 2
        for s in p.segments:
            assert any((z >> rc.sign_bit(s.tile, 25)) & 1 for z in zs[s.rot0:s.rot0 + s.nrot])


@pytest.mark.parametrize("real", [False, True])
def test_fibre_reference_against_the_oracle_on_the_whole_register(real):
    from openvqe_amd import synth
    n, seed, scale = 10, 99, 0.037
    rng = np.random.default_rng(5 + int(real))
    U = 0b1000110101                                     # the x masks live on five of the ten bits
    xs, zs, phis = [], [], []
    for k in range(14):
        x = 0
        while not x:
            x = int(rng.integers(0, 1 << n)) & U
        if k == 6 and not real:
            x = 0
        z = int(rng.integers(0, 1 << n))
        if real and not rc.popcount(x & z) & 1:
            z ^= x & -x
        xs.append(x); zs.append(z); phis.append(float(rng.uniform(-1, 1)))
    xs[0] = U
    if real and not rc.popcount(xs[0] & zs[0]) & 1:
        zs[0] ^= 1
    psi = synth.amplitudes(seed, np.arange(1 << n, dtype=np.uint64)) * scale
    if real:
        psi = psi.real.astype(complex)
    for x, z, p in zip(xs, zs, phis):
        psi = masks.rotate(psi, x, z, p)
    if real:
        assert np.abs(psi.imag).max() < 1e-16
    seen = set()
    for i in [0, 1, (1 << n) - 1, 1 << (n - 1)] + [int(v) for v in rng.integers(0, 1 << n, 12)]:
        G, want = rc.fibre_reference(seed, scale, i, xs, zs, phis, real)
        assert len(G) == 32 and i in G and all((int(v) ^ i) & ~U == 0 for v in G)
        assert np.abs(want - psi[G.astype(np.int64)]).max() < 1e-15
        seen.add(i & ~U)
    assert len(seen) > 4


@pytest.mark.parametrize("n,g", [(10, 0), (11, 2)])
def test_adjoint_reference_on_the_c_oracle_against_numpy(n, g):
    from tests.test_gpu_shard_gradient import _reference
    rng = np.random.default_rng(10 * n + g)
    nl = n - g
    psi, lam = random_state(rng, n), random_state(rng, n) * 1.7
    xs, zs, phis = [], [], []
    for k in range(20):
        x = 0 if k in (4, 5) else int(rng.integers(1, 1 << nl))
        xs.append(x); zs.append(int(rng.integers(0, 1 << n))); phis.append(float(rng.uniform(-1, 1)))
    w0, psi0, lam0 = _reference(psi, lam, xs, zs, phis, nl, g)
    w1, psi1, lam1 = rc.adjoint_reference_c(psi, lam, xs, zs, phis, nl, g)
    assert w0.shape == w1.shape == (1 << g, 20)
    assert np.abs(w0 - w1).max() < 1e-13 and np.abs(psi0 - psi1).max() < 1e-13 and np.abs(lam0 - lam1).max() < 1e-13
