"""The tile-cover kernels at their staging caps.  A staged chunk of a cover holds at most TILE_TERM_CAP = 512 terms and
TILE_APPLY_GROUPS = 128 pieces (openvqe_amd/csrc/sv_cover_host.hpp); a group with more terms is cut into pieces, a pass or sweep with
more pieces restages its LDS tables between barriers.  Production reaches both on the 31+ qubit partitioned registers only (the
diagonal group of a Jordan-Wigner Hamiltonian has 529 strings at 32 qubits; a molecular Hamiltonian on shards has more than 128 groups per
pass), so the sums of tests/cover_cases.py bring them down to 12..15 qubits:

  * across shards (ovqe_xsum_*: k_tile_cross, k_tile_cross_real, k_cross_small, k_cross_small_real), W shard handles of one GPU
    standing for the ranks and every partner chunk fed by hand: <H> per shard AS A COMPLEX NUMBER and sigma = (H + 0.3) psi, with real
    folded coefficients, imaginary ones (odd numbers of Y) and complex coefficients, on a dense state and on a state with one
    amplitude per shard (every other ket tile takes the zero exit);
  * on one register: <H> through k_tile_expect (entry walks with term lists above 512, the sparse-tile path that stages two host chunks
    per pass, with odd and even chunk counts), complex and real, and sigma through k_tile_apply.

The reference is the bit-mask oracle term by term on the whole register (oracle/masks.py; pinned against the C oracle's x-grouped sum
on these very sums in tests/test_cover_cases.py).  Bounds: 1e-11 |c|_1 on <H> (real and imaginary part), 1e-11 |c|_1 max|psi| sqrt(2^n) on
sigma (max-abs).  Not covered here: the non-temporal variants and k_tile_diag (25+ local qubits), k_tile_expect_compact, the listed-tile
form of k_tile_apply (no entry point used here passes a list), and the pool screen (tests/pool_cases.py has its own edge pool)."""
import numpy as np
import pytest

from oracle import masks
from tests import cover_cases as cc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def SV(gpu_lib):
    from openvqe_amd.backend import Statevector
    return Statevector


# (n, g, chunk_bits) -> (tile_bits, streaming_fallback) of ovqe_xsum_info: the smallest registers that reach each form
COMPLEX_CASES = [((13, 1, 10), (10, 0)),     # complex tiles of 2^10, two classes of x bits above the chunk
                 ((13, 1, 12), (12, 0)),     # the chunk is the shard: one pass of 5..6 staged chunks
                 ((14, 2, 11), (11, 0)),     # three partners, tiles of 2^11
                 ((15, 1, 12), (12, 0)),     # several tiles per chunk
                 ((12, 2, 8), (0, 1))]       # small form
REAL_CASES = [((13, 1, 11), (11, 0)),        # real tiles of 2^11
              ((14, 1, 13), (13, 0)),        # real tiles of 2^13
              ((12, 1, 9), (0, 1))]          # small form


def _cross_shard_case(SV, shape, form, builder, style, real):
    """<H> and sigma = (H + 0.3) psi of one sum on W = 2^g shard handles against the oracle; -> nothing, asserts"""
    import torch
    n, g, chunk_bits = shape
    nl, W = n - g, 1 << g
    ref = cc.reference(builder, n, nl, style, real)
    xs, zs, cs, l1 = ref["xs"], ref["zs"], ref["cs"], ref["l1"]
    csize, nchunks = 1 << chunk_bits, 1 << (nl - chunk_bits)
    with_expect = style != "complex"                       # <H> of a non-Hermitian sum is refused
    with_sigma = not (real and style != "symmetric")       # real storage holds sigma of a real-symmetric sum only
    distinct = cc.distinct_local_x(xs, zs, nl, even_y_only=real)
    tag = f"{shape} {builder}/{style}{' real' if real else ''}"
    shards = [SV(nl, n_global=g, shard_index=s) for s in range(W)]
    try:
        sids = None
        for name, psi, h0, hx in ref["states"]:
            host = [np.ascontiguousarray(p.real if real else p) for p in np.split(psi, W)]
            bufs = [torch.from_numpy(h.copy()).cuda() for h in host]
            outs = [torch.full((1 << nl,), 7.0, dtype=bufs[0].dtype, device="cuda") for _ in range(W)]   # (apply_local overwrites)
            for sv, b in zip(shards, bufs):
                sv.adopt_state(b.data_ptr())
                sv.set_option("real_state", 1 if real else 0)
            if sids is None:
                sids = [sv.xsum_create(xs, zs, cs, chunk_bits) for sv in shards]
            total, want_total = 0j, 0j
            for s, (sv, sid) in enumerate(zip(shards, sids)):
                info = sv.xsum_info(sid)
                partners = sv.xsum_partners(sid)
                assert (info["tile_bits"], info["streaming_fallback"]) == form, tag
                assert sorted(d for d, _ in partners) == sorted(distinct) and info["remote_groups"] == sum(distinct.values()), tag
                if name == "dense" and s == 0:
                    print(f"{tag}: form {form}, passes per partner {dict(partners)}, groups per partner {distinct}")
                # more groups than the passes can stage at once: by pigeonhole some pass of every partner has restaged.  (Between
                # real vectors the planner drops the odd-Y strings, about half the single-term groups of the "hermitian" sum: that
                # case is about the dropping; "symmetric" carries the restaging of the real kernels.)
                if builder == "staging" and form[0] and not (real and style == "hermitian"):
                    for d, passes in partners:
                        assert distinct[d] > cc.GROUP_CAP * passes, (tag, d, passes)
                sl = slice(s << nl, (s + 1) << nl)
                if with_expect:
                    local = sv.xsum_expect_local(sid)
                    for d, _ in partners:
                        for c in range(nchunks):
                            sv.xsum_expect_remote(sid, d, c, bufs[s ^ d][c * csize:(c + 1) * csize].data_ptr())
                    cross = sv.xsum_expect_finish(sid)
                    assert sv.xsum_expect_finish(sid) == 0j                       # the accumulator was reset
                    want_local, want_cross = np.vdot(psi[sl], h0[sl]), np.vdot(psi[sl], hx[sl])
                    got, want = local + cross, want_local + want_cross
                    if real and style == "hermitian":       # the odd-Y strings are left out: the reference's real part is what counts
                        want, want_cross = complex(want.real), complex(want_cross.real)
                    errs = (abs(got.real - want.real), abs(got.imag - want.imag), abs(local - want_local.real),
                            abs(cross.real - want_cross.real), abs(cross.imag - want_cross.imag))
                    print(f"{tag} {name} shard {s}: <H>_s = {got:.12f}, errors re/im {errs[0]:.2e}/{errs[1]:.2e} "
                          f"(local {errs[2]:.2e}, cross {errs[3]:.2e}/{errs[4]:.2e}), bound {1e-11 * l1:.2e}")
                    assert max(errs) <= 1e-11 * l1, (tag, name, s, got, want)
                    total += got
                    want_total += want
                if with_sigma:
                    sv.xsum_apply_local(sid, outs[s].data_ptr(), cc.IDENT)
                    for d, _ in partners:
                        for c in range(nchunks):
                            sv.xsum_apply_remote(sid, d, c, bufs[s ^ d][c * csize:(c + 1) * csize].data_ptr(), outs[s].data_ptr())
            torch.cuda.synchronize()
            if with_expect:
                assert abs(total.real - want_total.real) <= 1e-11 * l1 and abs(total.imag - want_total.imag) <= 1e-11 * l1, (tag, name)
            if with_sigma:
                want_sigma = cc.IDENT * psi + h0 + hx
                got_sigma = np.concatenate([o.cpu().numpy() for o in outs])
                err = np.abs(got_sigma - (want_sigma.real if real else want_sigma)).max()
                bound = 1e-11 * l1 * np.abs(psi).max() * np.sqrt(float(1 << n))
                print(f"{tag} {name}: max |sigma - oracle| = {err:.3e}, bound {bound:.3e}")
                assert err <= bound, (tag, name)
            for b, h in zip(bufs, host):
                assert np.array_equal(b.cpu().numpy(), h), (tag, name)             # the state was only read
    finally:
        for sv in shards:
            sv.set_option("real_state", 0)
            sv.close()


@pytest.mark.parametrize("style", cc.STYLES)
@pytest.mark.parametrize("builder", sorted(cc.BUILDERS))
@pytest.mark.parametrize("shape,form", COMPLEX_CASES)
def test_cross_shard_sums_at_the_staging_caps(SV, shape, form, builder, style):
    _cross_shard_case(SV, shape, form, builder, style, real=False)


@pytest.mark.parametrize("style", ["symmetric", "hermitian"])
@pytest.mark.parametrize("builder", sorted(cc.BUILDERS))
@pytest.mark.parametrize("shape,form", REAL_CASES)
def test_cross_shard_sums_at_the_staging_caps_real_flavour(SV, shape, form, builder, style):
    """float64 shards: "symmetric" <H> and sigma (the d = 0 cover of ovqe_xsum_apply_local runs the 600-string diagonal and the 530-string
    group through k_tile_cross_real with the shard as its one chunk), "hermitian" <H> only"""
    _cross_shard_case(SV, shape, form, builder, style, real=True)


# ---- one register -------------------------------------------------------------------------------------------------------------
N_REG = 14


def _register_states(rng, n, tile_bits, real=False):
    sparse = cc.sparse_state(rng, n, real)
    half = sparse.copy()
    half[((np.arange(1 << n) >> tile_bits) & 1) == 1] = 0.0         # every second tile (the tiles are the low bits here) emptied
    return [("dense", cc.dense_state(rng, n, real)), ("sparse", sparse), ("half_empty", half / np.linalg.norm(half))]


def _expect_on_register(sv, psi, xs, zs, cr, tile_bits):
    """<H> of the handle's state by ovqe_bilinear with tiles of 2^tile_bits (twice: bit-identical) and by the one-sweep-per-group kernel"""
    sv.set_state(psi)
    sv.set_option("tile_bits", tile_bits)
    tiled = sv.bilinear(xs, zs, cr)
    assert sv.bilinear(xs, zs, cr) == tiled
    sv.set_option("tile_bits", 0)
    plain = sv.bilinear(xs, zs, cr)
    sv.set_option("tile_bits", tile_bits)
    return tiled.real, plain.real


@pytest.mark.parametrize("style", ["symmetric", "hermitian"])
@pytest.mark.parametrize("tile_bits", [11, 12])
def test_register_expectation_with_term_lists_above_the_cap(SV, tile_bits, style):
    """k_tile_expect, complex: a dense state (entry walks; the merged term lists of the 600- and 530-string groups are split), a state with
    one amplitude in eight (every tile takes the sparse path) and the same with every second tile emptied; by ovqe_bilinear and by a
    planned sum's ovqe_xsum_expect_local, whose info reports that no group was left untiled"""
    n = N_REG
    rng = np.random.default_rng(100 * tile_bits + cc.STYLES.index(style))
    xs, zs, cs = cc.register_sum(rng, n, style)
    cr, l1 = np.ascontiguousarray(cs.real), float(np.abs(cs).sum())
    with SV(n) as sv:
        sv.set_option("force_path", 2)
        sv.set_option("tile_bits", tile_bits)
        sid = sv.xsum_create(xs, zs, cr, 12)
        for name, psi in _register_states(rng, n, tile_bits):
            want = masks.expectation(psi, xs, zs, cr)
            tiled, plain = _expect_on_register(sv, psi, xs, zs, cr, tile_bits)
            planned = sv.xsum_expect_local(sid)
            info = sv.xsum_info(sid)                         # (the cover is built at the first evaluation)
            assert info["local_untiled_groups"] == 0 and info["local_tile_sweeps"] >= 1 and sv.xsum_partners(sid) == []
            errs = abs(tiled - want), abs(tiled - plain), abs(planned - want)
            print(f"tile_bits {tile_bits} {style} {name}: <H> = {tiled:.12f}, |tiled - oracle| = {errs[0]:.2e}, |tiled - untiled| = "
                  f"{errs[1]:.2e}, |planned - oracle| = {errs[2]:.2e}, bound {1e-11 * l1:.2e}, sweeps {info['local_tile_sweeps']}")
            assert max(errs) <= 1e-11 * l1, (name, tiled, plain, planned, want)
            assert sv.xsum_expect_local(sid) == planned


@pytest.mark.parametrize("low_groups", [100, 230, 360])
def test_sparse_tile_path_with_odd_and_even_chunk_counts(SV, low_groups):
    """the sparse path of k_tile_expect stages two host chunks per pass, the last pass of an odd count one chunk twice over
    (achunks[min(ch + 1, sw.a1 - 1)]): low-mask families of 100, 230 and 360 groups give the one sweep 182, 302 and 439 pieces of 1250, 1380
    and 1510 terms, staged as 3, 4 and 5 host chunks"""
    n, tile_bits = N_REG, 11
    rng = np.random.default_rng(low_groups)
    xs, zs, cs = cc.register_sum(rng, n, "hermitian", low_groups)
    cr, l1 = np.ascontiguousarray(cs.real), float(np.abs(cs).sum())
    psi = cc.sparse_state(rng, n)
    want = masks.expectation(psi, xs, zs, cr)
    with SV(n) as sv:
        sv.set_option("force_path", 2)
        tiled, plain = _expect_on_register(sv, psi, xs, zs, cr, tile_bits)
    print(f"{low_groups} low groups: |tiled - oracle| = {abs(tiled - want):.2e}, |tiled - untiled| = {abs(tiled - plain):.2e}, "
          f"bound {1e-11 * l1:.2e}")
    assert abs(tiled - want) <= 1e-11 * l1 and abs(tiled - plain) <= 1e-11 * l1


def test_register_expectation_real_flavour(SV):
    """k_tile_expect<REAL> (tiles of 2^12 doubles) on a 15-qubit float64 register: the dense real state and the one-in-eight sparse one"""
    import torch
    n = 15
    rng = np.random.default_rng(15)
    xs, zs, cs = cc.register_sum(rng, n, "symmetric")
    cr, l1 = np.ascontiguousarray(cs.real), float(np.abs(cs).sum())
    with SV(n) as sv:
        sid = None
        for name, psi in _register_states(rng, n, 12, real=True)[:2]:
            buf = torch.from_numpy(np.ascontiguousarray(psi.real)).cuda()
            sv.adopt_state(buf.data_ptr())
            sv.set_option("real_state", 1)
            if sid is None:
                sid = sv.xsum_create(xs, zs, cr, 12)
            want = masks.expectation(psi, xs, zs, cr)
            got = sv.xsum_expect_local(sid)
            info = sv.xsum_info(sid)
            assert info["local_untiled_groups"] == 0 and info["local_tile_sweeps"] >= 1
            print(f"real {name}: <H> = {got:.12f}, |got - oracle| = {abs(got - want):.2e}, bound {1e-11 * l1:.2e}")
            assert abs(got - want) <= 1e-11 * l1 and sv.xsum_expect_local(sid) == got
            assert np.array_equal(buf.cpu().numpy(), psi.real)
        sv.set_option("real_state", 0)


@pytest.mark.parametrize("style", cc.STYLES)
def test_register_sigma_through_the_tile_sweeps(SV, style):
    """k_tile_apply (tiles of 2^11, forced on a register this small by apply_min_tiles = 1): sigma = (H + 0.3) psi of a sweep whose pieces
    fill several staged chunks, on a dense state and on a sparse one with every second tile empty (the zero-tile exit still has to
    write ident * psi in the first sweep); out starts as 7.0 everywhere"""
    import torch
    n, tile_bits = N_REG, 11
    rng = np.random.default_rng(40 + cc.STYLES.index(style))
    xs, zs, cs = cc.register_sum(rng, n, style)
    l1 = float(np.abs(cs).sum())
    with SV(n) as sv:
        sv.set_option("force_path", 2)
        sv.set_option("apply_min_tiles", 1)
        sv.set_option("tile_bits", tile_bits)
        sid = sv.xsum_create(xs, zs, cs, 12)
        states = _register_states(rng, n, tile_bits)
        for name, psi in (states[0], states[2]):
            buf = torch.from_numpy(psi.copy()).cuda()
            out = torch.full((1 << n,), 7.0, dtype=torch.complex128, device="cuda")
            sv.adopt_state(buf.data_ptr())
            sv.xsum_apply_local(sid, out.data_ptr(), cc.IDENT)
            torch.cuda.synchronize()
            info = sv.xsum_info(sid)
            assert info["local_untiled_groups"] == 0 and info["local_tile_sweeps"] >= 1
            want = cc.IDENT * psi + masks.apply_pauli_sum(psi, xs, zs, cs)
            err, bound = np.abs(out.cpu().numpy() - want).max(), 1e-11 * l1 * np.abs(psi).max() * np.sqrt(float(1 << n))
            print(f"{style} {name}: max |sigma - oracle| = {err:.3e}, bound {bound:.3e}")
            assert err <= bound
            assert np.array_equal(buf.cpu().numpy(), psi)
