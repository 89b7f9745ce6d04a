"""The backward step of the adjoint method on the device — ``ovqe_adjoint_rotations``: k_tile_adjoint (psi and lambda tiles in
LDS, one pass per tile segment) and the streaming kernels (one pass per same-x run of at most 16 rotations) — straight through the
binding against numpy, on plain handles and on shard handles; then ``ShardedStatevector.program_energy_gradient`` and
``PartitionedStatevector.energy_gradient`` on HIP shards (every rank's shard on this GPU, gloo), same checks and the same bound as
tests/test_shard_gradient.py: |dE|, max |d grad| < 1e-11 * ||H||_1."""
import numpy as np
import pytest
import torch.multiprocessing as mp

from oracle import masks
from tests.test_distributed import _free_port

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def SV(gpu_lib):
    from openvqe_amd.backend import Statevector
    return Statevector


def _lists(rng, n, nl, kind):
    """rotation lists with x on the nl local bits and z anywhere in the n-bit register"""
    xs, zs, phis = [], [], []

    def run(x, reps):
        for _ in range(reps):
            xs.append(int(x)); zs.append(int(rng.integers(0, 1 << n))); phis.append(float(rng.uniform(-1, 1)))

    if kind == "segments":        # low-weight strings, several same-x runs per tile; a wide string and a diagonal run in between
        for k in range(30):
            if k % 10 == 9:
                run(rng.integers(1, 1 << nl), 1)
            elif k % 7 == 3:
                run(0, 1 + int(rng.integers(0, 3)))
            else:
                bits = rng.choice(nl, int(rng.choice([1, 2, 4])), replace=False)
                run(sum(1 << int(b) for b in bits), 1 + int(rng.integers(0, 3)))
    elif kind == "long_run":      # same-x runs longer than the 16 rotations a streaming pass takes: a wide mask, and one inside a segment
        run((1 << (nl - 1)) | (1 << (nl - 3)) | 5, 37)
        run(0b110, 21)
        run(0b1001, 3)
    elif kind == "diagonal":
        run(0, 19)
    elif kind == "single":
        run((1 << (nl - 1)) | 1, 1)
    else:
        raise ValueError(kind)
    return xs, zs, phis


def _reference(psi, lam, xs, zs, phis, nl, g):
    """numpy: per shard the sums w[s, r] = Im <lam_s|P_r|psi_s>, both vectors un-rotated last to first"""
    psi, lam = psi.copy(), lam.copy()
    w = np.zeros((1 << g, len(xs)))
    for r in range(len(xs) - 1, -1, -1):
        x, z, p = xs[r], zs[r], phis[r]
        for s in range(1 << g):
            sl = slice(s << nl, (s + 1) << nl)
            a, l = psi[sl], lam[sl]
            pa = masks.pauli_apply(a, x, z, index_offset=s << nl)
            pl = masks.pauli_apply(l, x, z, index_offset=s << nl)
            w[s, r] = np.vdot(l, pa).imag
            psi[sl] = np.cos(p) * a + 1j * np.sin(p) * pa
            lam[sl] = np.cos(p) * l + 1j * np.sin(p) * pl
    return w, psi, lam


def _runs(xs, cap=16):
    total, a = 0, 0
    while a < len(xs):
        b = a + 1
        while b < len(xs) and xs[b] == xs[a]:
            b += 1
        total += -(-(b - a) // cap)
        a = b
    return total


@pytest.mark.parametrize("n,g,kind,tile_bits", [
    (14, 0, "segments", -1), (15, 0, "segments", 12), (15, 1, "segments", -1), (16, 2, "segments", 12), (16, 2, "segments", 11),
    (15, 1, "segments", 0), (15, 0, "long_run", -1), (16, 2, "long_run", 12), (14, 0, "diagonal", -1), (15, 1, "single", -1),
    (10, 0, "segments", -1), (12, 2, "long_run", -1)])
def test_adjoint_rotations_against_numpy(SV, n, g, kind, tile_bits):
    import torch
    from tests.util import random_state
    rng = np.random.default_rng(4321 + 100 * n + 10 * g + len(kind))
    nl = n - g
    psi, lam = random_state(rng, n), random_state(rng, n) * 1.7
    xs, zs, phis = _lists(rng, n, nl, kind)
    w_ref, psi_ref, lam_ref = _reference(psi, lam, xs, zs, phis, nl, g)
    for s in range(1 << g):                                    # (every shard index, the non-zero ones included)
        with SV(nl, n_global=g, shard_index=s) as sv:
            sv.set_option("adjoint_tile_bits", tile_bits)
            sv.set_state(psi[s << nl:(s + 1) << nl])
            lam_dev = torch.from_numpy(lam[s << nl:(s + 1) << nl].copy()).to("cuda:0")
            w = sv.adjoint_rotations(lam_dev.data_ptr(), xs, zs, phis)
            passes, nbytes = sv.last_passes()
            got_psi, got_lam = sv.get_state(), lam_dev.cpu().numpy()
        err = (np.abs(w - w_ref[s]).max(), np.abs(got_psi - psi_ref[s << nl:(s + 1) << nl]).max(),
               np.abs(got_lam - lam_ref[s << nl:(s + 1) << nl]).max())
        print(f"n {n} g {g} shard {s} {kind} tile_bits {tile_bits}: passes {passes} of {_runs(xs)} runs, errors {err}")
        assert max(err) < 1e-12
        assert nbytes == 64 * (1 << nl) * passes
        tiles = tile_bits != 0 and nl >= (12 if tile_bits == 12 else 11) + 2
        if tiles and kind in ("segments", "long_run"):
            assert passes < _runs(xs)                           # tile segments: several runs per pass
        else:
            assert passes == _runs(xs)                          # the streaming kernels: one pass per run of at most 16


def test_adjoint_rotations_refusals(SV):
    import torch
    from openvqe_amd._lib import BackendError
    with SV(12, n_global=1, shard_index=1) as sv:
        sv.init_basis(1 << 12)
        lam = torch.zeros(1 << 12, dtype=torch.complex128, device="cuda:0")
        with pytest.raises(BackendError, match="state buffer"):
            sv.adjoint_rotations(sv.state_ptr(), [3], [1], [0.1])
        with pytest.raises(BackendError, match="global"):
            sv.adjoint_rotations(lam.data_ptr(), [1 << 12], [1], [0.1])       # x on the rank bit
        with pytest.raises(BackendError, match="beyond the register"):
            sv.adjoint_rotations(lam.data_ptr(), [3], [1 << 13], [0.1])
        sv.set_option("real_state", 1)
        with pytest.raises(BackendError, match="real_state"):
            sv.adjoint_rotations(lam.data_ptr(), [3], [1], [0.1])
        sv.set_option("real_state", 0)
        assert np.abs(sv.adjoint_rotations(lam.data_ptr(), [3], [1], [0.1])).max() == 0.0     # (lambda = 0)


# shards of 13 and more local qubits take tile segments, smaller ones the streaming kernels only
@pytest.mark.parametrize("world,n,chunk_bits", [(2, 15, 10), (4, 16, 10), (8, 16, 10), (8, 15, 9), (2, 17, 12)])
def test_adjoint_gradient_on_hip_shards(gpu_lib, world, n, chunk_bits):
    from tests.test_shard_gradient import check_gradient_cases, gradient_worker, launch
    res = launch(gradient_worker, world, (n, 977 + n + world, "hip", chunk_bits))
    check_gradient_cases(res, world, n)
    for r in res:
        passes = r["counters"]["adjoint_passes"]
        print(f"world {world} n {n}: n_local {r['n_local']} adjoint passes {passes}, same-x runs {r['chunks']}")
        assert r["counters"]["adjoint_bytes"] == 64 * (1 << r["n_local"]) * passes
        if r["n_local"] >= 13:
            assert 0 < passes < r["chunks"]
        else:
            assert passes == r["chunks"]


def test_adjoint_gradient_through_the_evaluator_on_hip_shards(gpu_lib):
    """UCCEvaluator.energy_gradient and EnergyUCC._minimize with adjoint_gradient = True, register partitioned over two HIP shards"""
    from tests.test_shard_gradient import api_worker, check_api, single_process_api
    flows = ("gradient", "minimize")
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=api_worker, args=(r, 2, port, "hip", flows, out)) for r in range(2)]
    for p in procs:
        p.start()
    got = out.get(timeout=900)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    check_api(got, single_process_api(flows))
