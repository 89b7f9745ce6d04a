"""sigma = H psi on 8-byte amplitudes straight through the binding (option "real_state"): ovqe_xsum_apply_local / _remote on W shard
handles of one GPU standing for the ranks, every form the real cover instantiates — the small kernel (chunks below 2^11 doubles)
and tiles of 2^11 / 2^12 / 2^13 doubles across shards; inside a shard the d = 0 groups run through the same kernels with the shard
as its own chunk (small below 11 local qubits, tiles of 2^11 .. 2^13 above) — against the bit-mask oracle on the whole register.
Then the Lanczos vector operations (ovqe_vec_*) and the real fill of ovqe_randomize."""
import numpy as np
import pytest

from oracle import masks

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def SV(gpu_lib):
    from openvqe_amd.backend import Statevector
    return Statevector


def real_symmetric_sum(rng, n, g, T=48):
    """seeded strings with an even number of Y and real coefficients: an x = 0 group, groups inside the shard, x on one and (g > 1)
    on several rank bits, x bits above and below every chunk size in use"""
    nl = n - g
    xs = np.array([int(v) for v in rng.integers(0, 1 << n, T)], np.uint64)
    xs[:6] = 0
    xs[6:14] &= np.uint64((1 << nl) - 1)
    xs[14:18] = xs[14]                                             # a group of four terms
    xs[18] = np.uint64(1 << (n - 1))                               # one rank bit alone
    xs[19] = np.uint64(((1 << g) - 1) << nl)                       # every rank bit
    xs[20] = np.uint64((1 << nl) | 1 | (1 << (nl - 1)))            # lowest rank bit, top and bottom local bit
    zs = np.array([int(v) for v in rng.integers(0, 1 << n, T)], np.uint64)
    odd = np.array([bin(int(x) & int(z)).count("1") % 2 == 1 for x, z in zip(xs, zs)])
    zs = np.where(odd & (xs != 0), zs ^ (xs & (~xs + np.uint64(1))), zs)
    assert all(bin(int(x) & int(z)).count("1") % 2 == 0 for x, z in zip(xs, zs))
    return xs, zs, rng.normal(size=T)


# (W, n, chunk_bits) -> (tile bits, small) of the remote cover as ovqe_xsum_info reports them
CASES = [((2, 10, 6), (0, 1)), ((2, 12, 8), (0, 1)), ((4, 15, 10), (0, 1)), ((2, 13, 11), (11, 0)), ((2, 15, 12), (12, 0)),
         ((2, 17, 13), (13, 0)), ((8, 16, 10), (0, 1))]


@pytest.mark.parametrize("shape,form", CASES)
def test_real_apply_against_oracle(SV, shape, form):
    import torch
    W, n, chunk_bits = shape
    g = W.bit_length() - 1
    nl = n - g
    rng = np.random.default_rng(1000 * n + 10 * W + chunk_bits)
    xs, zs, cs = real_symmetric_sum(rng, n, g)
    ident = 0.3
    dense_vec = rng.normal(size=1 << n)
    dense_vec /= np.linalg.norm(dense_vec)
    single = np.zeros(1 << n)
    single[int(rng.integers(0, 1 << n))] = 1.7                      # one non-zero amplitude: every other ket tile takes the zero exit
    csize = 1 << chunk_bits
    shards = [SV(nl, n_global=g, shard_index=s) for s in range(W)]
    try:
        sids = None
        for psi in (dense_vec, single):
            want = ident * psi + masks.apply_pauli_sum(psi.astype(complex), xs, zs, cs)
            assert np.abs(want.imag).max() == 0.0
            bufs = [torch.from_numpy(psi[s << nl:(s + 1) << nl].copy()).cuda() for s in range(W)]
            outs = [torch.full((1 << nl,), 7.0, dtype=torch.float64, device="cuda") for _ in range(W)]   # (apply_local overwrites)
            for sv, b in zip(shards, bufs):
                sv.adopt_state(b.data_ptr())
                sv.set_option("real_state", 1)
            if sids is None:
                sids = [sv.xsum_create(xs, zs, cs, chunk_bits) for sv in shards]
            for s, (sv, sid) in enumerate(zip(shards, sids)):
                info = sv.xsum_info(sid)
                assert (info["tile_bits"], info["streaming_fallback"]) == form
                partners = sv.xsum_partners(sid)
                assert len(partners) == len({int(x) >> nl for x in xs if int(x) >> nl})
                sv.xsum_apply_local(sid, outs[s].data_ptr(), ident)
                for d, _ in partners:
                    ket = bufs[s ^ d]
                    for c in range(1 << (nl - chunk_bits)):
                        sv.xsum_apply_remote(sid, d, c, ket[c * csize:(c + 1) * csize].data_ptr(), outs[s].data_ptr())
            torch.cuda.synchronize()
            got = np.concatenate([o.cpu().numpy() for o in outs])
            err = np.abs(got - want.real).max()
            bound = 1e-12 * np.abs(cs).sum() * np.abs(psi).max()
            print(f"{shape}: max |sigma - oracle| = {err:.3e}, bound {bound:.3e}")
            assert err <= bound
            for b, psi_s in zip(bufs, np.split(psi, W)):
                assert np.array_equal(b.cpu().numpy(), psi_s)          # the state was only read
    finally:
        for sv in shards:
            sv.close()


def test_real_apply_refusals(SV):
    """a sum that leaves the real vectors (one odd-Y string; one complex coefficient) and an out buffer that is, or overlaps, the
    state: OVQE_ERR_STATE (-5), nothing written"""
    import torch
    from openvqe_amd._lib import BackendError
    nl, g = 11, 1
    rng = np.random.default_rng(5)
    xs, zs, cs = real_symmetric_sum(rng, nl + g, g)
    buf = torch.from_numpy(rng.normal(size=1 << nl)).cuda()
    out = torch.zeros(1 << nl, dtype=torch.float64, device="cuda")
    chunk = torch.zeros(1 << 8, dtype=torch.float64, device="cuda")
    keep = buf.clone()
    with SV(nl, n_global=g, shard_index=1) as sv:
        sv.adopt_state(buf.data_ptr())
        sv.set_option("real_state", 1)
        zodd = zs.copy()
        zodd[20] ^= np.uint64(1)                                     # x has bit 0 there: one more Y
        assert bin(int(xs[20]) & int(zodd[20])).count("1") % 2 == 1
        for bad in (sv.xsum_create(xs, zodd, cs, 8), sv.xsum_create(xs, zs, cs * (1.0 + 0.5j), 8)):
            with pytest.raises(BackendError, match=r"error -5: .*real-symmetric"):
                sv.xsum_apply_local(bad, out.data_ptr(), 0.0)
            with pytest.raises(BackendError, match=r"error -5: .*real-symmetric"):
                sv.xsum_apply_remote(bad, 1, 0, chunk.data_ptr(), out.data_ptr())
        sid = sv.xsum_create(xs, zs, cs, 8)
        with pytest.raises(BackendError, match=r"error -5: .*overlaps the state"):
            sv.xsum_apply_local(sid, buf.data_ptr(), 0.0)
        with pytest.raises(BackendError, match=r"error -5: .*overlaps the state"):
            sv.xsum_apply_remote(sid, 1, 0, chunk.data_ptr(), buf.data_ptr())
        torch.cuda.synchronize()
        assert torch.equal(buf, keep) and float(out.abs().max()) == 0.0
        sv.set_option("real_state", 0)


@pytest.mark.parametrize("n_global,shard", [(0, 0), (2, 1)])
@pytest.mark.parametrize("real", [False, True])
def test_lanczos_vector_operations(SV, n_global, shard, real):
    """ovqe_vec_dot / _lanczos_update / _scale / _axpy on caller-held buffers of the handle's storage against numpy"""
    import torch
    nl = 11
    rng = np.random.default_rng(17 + n_global + 2 * real)
    draw = (lambda: rng.normal(size=1 << nl)) if real else (lambda: rng.normal(size=1 << nl) + 1j * rng.normal(size=1 << nl))
    a, b, c = draw(), draw(), draw()
    rel = lambda got, want: abs(got - want) / max(abs(want), 1e-300)
    state = torch.zeros(1 << nl, dtype=torch.float64 if real else torch.complex128, device="cuda")
    with SV(nl, n_global=n_global, shard_index=shard) as sv:
        sv.adopt_state(state.data_ptr())
        sv.set_option("real_state", 1 if real else 0)
        ta, tb, tc = (torch.from_numpy(v.copy()).cuda() for v in (a, b, c))
        got = sv.vec_dot(ta.data_ptr(), tb.data_ptr())
        assert rel(got, np.vdot(a, b)) < 1e-13 and (not real or got.imag == 0.0)
        for vprev, tprev in ((c, tc), (None, None)):
            w = a - 0.37 * b - (0.0 if vprev is None else -1.21 * vprev)
            tw = ta.clone()
            n2 = sv.vec_lanczos_update(tw.data_ptr(), tb.data_ptr(), None if tprev is None else tprev.data_ptr(), 0.37, -1.21)
            torch.cuda.synchronize()
            assert rel(n2, np.vdot(w, w).real) < 1e-13
            assert np.abs(tw.cpu().numpy() - w).max() < 1e-13 * np.abs(w).max()
        ty = ta.clone()
        sv.vec_scale(ty.data_ptr(), -0.75)
        sv.vec_axpy(ty.data_ptr(), tb.data_ptr(), 2.5)
        tz = tc.clone()
        sv.vec_axpy(tz.data_ptr(), tb.data_ptr(), -3.0, overwrite=True)
        torch.cuda.synchronize()
        want = -0.75 * a + 2.5 * b
        assert np.abs(ty.cpu().numpy() - want).max() < 1e-13 * np.abs(want).max()
        assert np.array_equal(tz.cpu().numpy(), -3.0 * b)
        assert torch.equal(tb, torch.from_numpy(b).cuda())
        sv.set_option("real_state", 0)


def test_real_random_fill_is_the_real_part_and_partition_independent(SV):
    """ovqe_randomize under "real_state": 2^n_local doubles = the real parts of the complex fill at the same global indices
    (openvqe_amd/synth.py), nothing written past them; four shards side by side equal one 13-qubit handle bit for bit"""
    import torch
    from openvqe_amd import synth
    nl, g, seed = 11, 2, 20250227
    parts = []
    for s in range(1 << g):
        buf = torch.full((2 << nl,), 5.0, dtype=torch.float64, device="cuda")     # (twice the size: the second half must stay)
        with SV(nl, n_global=g, shard_index=s) as sv:
            sv.adopt_state(buf.data_ptr())
            sv.set_option("real_state", 1)
            assert sv.randomize(seed, 1.0) == 1.0
            re = synth.amplitudes(seed, np.arange(1 << nl, dtype=np.uint64) | np.uint64(s << nl)).real
            host = buf.cpu().numpy()
            assert np.array_equal(host[:1 << nl], re) and np.all(host[1 << nl:] == 5.0)
            assert abs(sv.norm2() - (re ** 2).sum()) < 1e-13 * (re ** 2).sum()
            if s == 1:       # the shard's own norm: scale = 1 / |re|
                scale = sv.randomize(seed, 0.0)
                assert abs(scale - 1.0 / np.sqrt((re ** 2).sum())) < 1e-13 * scale
                assert np.abs(buf.cpu().numpy()[:1 << nl] - re * scale).max() < 1e-15 and abs(sv.norm2() - 1.0) < 1e-13
                sv.randomize(seed, 1.0)
                host = buf.cpu().numpy()
            parts.append(host[:1 << nl].copy())
            sv.set_option("real_state", 0)
    whole = torch.zeros(1 << (nl + g), dtype=torch.float64, device="cuda")
    with SV(nl + g) as sv:
        sv.adopt_state(whole.data_ptr())
        sv.set_option("real_state", 1)
        sv.randomize(seed, 1.0)
        assert np.array_equal(whole.cpu().numpy(), np.concatenate(parts))
        sv.set_option("real_state", 0)
