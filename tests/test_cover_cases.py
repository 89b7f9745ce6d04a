"""The preconditions of tests/test_gpu_cover_caps.py that need no GPU: the sums of tests/cover_cases.py hold what their docstrings
claim (distinct masks, groups above the term cap that no merging shrinks, the coefficient classes), and the reference the GPU tests
compare with — the bit-mask oracle, term by term — agrees with the C oracle's x-grouped evaluation to a tenth of the GPU bound."""
from collections import Counter

import numpy as np
import pytest

from oracle import cref, masks
from tests import cover_cases as cc

GEOMETRIES = [(13, 12), (14, 12), (12, 10)]


def _groups(xs):
    return Counter(int(x) for x in xs)


@pytest.mark.parametrize("style", cc.STYLES)
@pytest.mark.parametrize("n,n_local", GEOMETRIES)
def test_staging_sum_holds_its_claims(n, n_local, style):
    xs, zs, cs = cc.staging_sum(np.random.default_rng(n + n_local), n, n_local, style)
    assert xs.dtype == zs.dtype == np.uint64 and cs.dtype == np.complex128 and len(xs) == len(zs) == len(cs)
    assert int((xs | zs).max()) < 1 << n
    lmask, top = (1 << n_local) - 1, 1 << (n_local - 1)
    by_d = {}
    for x in xs:
        by_d.setdefault(int(x) >> n_local, []).append(int(x) & lmask)
    assert sorted(by_d) == list(range(1 << (n - n_local)))
    for d, lx in by_d.items():
        if d == 0:
            continue
        count = Counter(lx)
        low = [x for x in count if x < 1 << 8]
        assert len(low) == 200 and sorted(x ^ top for x in count if x & top) == sorted(low)      # two classes of 200 distinct masks
        assert sorted(count.values()) == [1] * 399 + [531]                                        # one group past the term cap
        assert count[lx[0]] == 531 and lx[0] < 1 << 8
        assert cc.distinct_local_x(xs, zs, n_local)[d] == 400
    inside = (xs >> np.uint64(n_local)) == 0
    lx, lz = xs[inside], zs[inside]
    count = _groups(lx)
    assert count[0] == 600 and len({int(z) for z in lz[lx == 0]}) == 600                          # diagonal: pairwise distinct z
    assert count[0b101] == 530
    assert len({int(z) & ~0b101 for z in lz[lx == 0b101]}) == 530 > cc.TERM_CAP                   # no merge brings it under the cap
    singles = [x for x, c in count.items() if x not in (0, 0b101)]
    assert len(singles) == 230 > cc.GROUP_CAP and all(count[x] == 1 and x < 1 << 8 for x in singles)
    _check_style(xs, zs, cs, style)


@pytest.mark.parametrize("style", cc.STYLES)
@pytest.mark.parametrize("n,n_local", GEOMETRIES)
def test_geometry_sum_holds_its_claims(n, n_local, style):
    xs, zs, cs = cc.geometry_sum(np.random.default_rng(3 * n + n_local), n, n_local, style)
    assert len(xs) == 80 and int((xs | zs).max()) < 1 << n
    count = _groups(xs)
    assert count[0] == 6 and sum(1 for c in count.values() if c >= 3) >= 4                        # repeated masks
    ds = {int(x) >> n_local for x in xs}
    assert ds == set(range(1 << (n - n_local)))                                                   # every partner, and the shard itself
    assert any(int(x) >> n_local and int(x) & (1 << (n_local - 1)) for x in xs)                   # a bit above every chunk
    _check_style(xs, zs, cs, style)


@pytest.mark.parametrize("style,low_groups", [(s, 230) for s in cc.STYLES] + [("hermitian", 100), ("hermitian", 360)])
def test_register_sum_holds_its_claims(style, low_groups):
    n = 14
    xs, zs, cs = cc.register_sum(np.random.default_rng(low_groups), n, style, low_groups)
    assert all(cc.popcount(int(x) | 3) <= 10 for x in xs)                                         # every group fits a tile of 2^10 and up
    count = _groups(xs[:-20])
    assert count[0] == 600 and count[0b101] == 530 and len(count) == low_groups + 2
    assert len({int(z) & ~0b101 for x, z in zip(xs[:-20], zs[:-20]) if int(x) == 0b101}) == 530
    assert all(0 < int(x) < 1 << 8 for x in xs[-20:]) and np.all(cs[-20:].imag == 0.0)
    assert cc.odd_y(xs[-20:], zs[-20:]).any()                                                     # z as drawn, whatever the style
    _check_style(xs[:-20], zs[:-20], cs[:-20], style)


def _check_style(xs, zs, cs, style):
    odd = cc.odd_y(xs, zs)
    if style == "symmetric":
        assert not odd.any() and np.all(cs.imag == 0.0)
    elif style == "hermitian":
        assert odd.mean() >= 0.2 and np.all(cs.imag == 0.0)
    else:
        assert np.count_nonzero(cs.imag) == len(cs) and odd.any()
    assert 0.5 * len(cs) < np.abs(cs).sum()                                                       # N(0, 1): not scaled down


@pytest.mark.parametrize("style", ["symmetric", "hermitian"])
@pytest.mark.parametrize("builder", sorted(cc.BUILDERS))
def test_the_two_references_agree_within_a_tenth_of_the_gpu_bound(builder, style):
    """13 qubits, random state: <H> term by term (oracle.masks) against the C oracle's x-grouped sum; the GPU bound is 1e-11 |c|_1"""
    n, n_local = 13, 12
    rng = np.random.default_rng(13)
    xs, zs, cs = cc.BUILDERS[builder](rng, n, n_local, style)
    psi = cc.dense_state(rng, n)
    want = masks.expectation(psi, xs, zs, cs.real)
    sx, sz, sc = cref.sort_by_x(xs, zs, np.ascontiguousarray(cs.real))
    got = cref.lib().orc_expectation_grouped(np.ascontiguousarray(psi), n, len(sx), sx, sz, sc)
    err, bound = abs(got - want), 0.1 * 1e-11 * np.abs(cs).sum()
    print(f"{builder}/{style}: |masks - grouped| = {err:.3e}, a tenth of the GPU bound {bound:.3e}")
    assert err <= bound


def test_states_and_shared_reference():
    n, n_local = 13, 12
    ref = cc.reference("geometry", n, n_local, "hermitian")
    assert cc.reference("geometry", n, n_local, "hermitian") is ref                               # computed once
    (_, dense, h0, hx), (_, single, s0, sx) = ref["states"]
    assert not dense.flags.writeable and not ref["cs"].flags.writeable
    assert abs(np.linalg.norm(dense) - 1.0) < 1e-14 and abs(np.linalg.norm(single) - 1.0) < 1e-14
    assert [np.count_nonzero(s) for s in np.split(single, 2)] == [1, 1]
    assert abs(np.vdot(single, sx)) > 0.0                                                         # a string connects the two amplitudes
    want = masks.apply_pauli_sum(dense, ref["xs"], ref["zs"], ref["cs"])
    assert np.abs(h0 + hx - want).max() < 1e-13 * ref["l1"]
    sp = cc.sparse_state(np.random.default_rng(1), 14, empty_block_bits=11)
    blocks = [np.count_nonzero(b) for b in np.split(sp, 8)]
    assert all(0 < b <= 2048 // 4 for b in blocks[0::2]) and blocks[1::2] == [0] * 4
