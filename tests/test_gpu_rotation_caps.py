"""The rotation-list kernels at their table caps and in the forms the large shards launch.  ``ovqe_apply_pauli_rotations`` (k_tile_sweep
on complex amplitudes and, under "real_state", on doubles; what fits no tile through launch_rot_run / k_rot_pairs_real) and
``ovqe_adjoint_rotations`` (k_tile_adjoint; k_adjoint_pairs / k_adjoint_diag in chunks of 16) cut their list with build_tile_plan.  The
lists of tests/rotation_cases.py put that cut on each side of the caps — a segment filled exactly to TILE_ROT_CAP = 256 (forward) or
tile_adj_rot_cap = 128 / 256 (backward), a segment closed by the cap, a same-x run longer than the cap, a second segment with rot0 > 0
behind a full table — and the pass counters of the product are compared with the Python model of the cut, which is what proves that
a boundary was reached.

  A  backward caps: 13 / 14 local qubits, tiles of 2^11 / 2^12, plain and shard handles, against numpy
  B  forward caps: complex tiles of 2^10..2^12 and real tiles of 2^11..2^13, against oracle/masks.py
  C  one workgroup of k_tile_adjoint walks several tiles: 21 local qubits (the grid is sized to the CUs: the smallest shard that gives a
     workgroup a second trip, with a sign of the sums that differs between its tiles), against the C oracle
  D  the non-temporal instantiations of 25+ local qubits with the automatic tile size — k_tile_sweep<12, 512, true, false>,
     k_tile_sweep<13, 512, true, true>, k_tile_adjoint<12, 512, true> —: forward on the synthetic state against the rotations applied on
     whole fibres of sampled indices (no host copy of the state), backward against the C oracle

Bounds: max-abs 1e-12 on amplitudes and sums with |psi| = 1, |lambda| = 1.7 (the bounds of tests/test_gpu_shard_gradient.py and
tests/test_gpu_tile.py); D forward 8 R eps max|a| (the single-rotation bound of tests/test_gpu_nccl.py, one rounding of that size per
rotation).  The backward kernel uses no atomics: a second call on the same inputs must return the same bits.

Wall time per case, measured on an MI355X host with 16 CPUs (the first case of a process also loads the library, 1.5 s): A 0.02 .. 0.3 s
(the largest at 14 + 2 qubits, the numpy reference over four shards), B 0.01 .. 0.05 s, C 0.3 .. 0.6 s at 21 and 22 qubits, D forward
0.1 s (real; complex 1.7 s as the first case of its process), D backward 1.1 s — dominated by the CPU references; the 132 cases take 28 s
together and none is among the 60 slowest of the suite (3.4 s).

Not covered here: OP_TAB entries at the cap (they arise in compiled programs only; the kernel code behind the table is shared); the
grid-stride trips of k_adjoint_pairs / k_adjoint_diag (26+ local qubits and a reference of the whole register); 32+ local qubits."""
import math

import numpy as np
import pytest

from oracle import masks
from tests import rotation_cases as rc
from tests.util import random_state

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def SV(gpu_lib):
    from openvqe_amd.backend import Statevector
    return Statevector


def _states(n, seed):
    rng = np.random.default_rng(seed)
    return random_state(rng, n), random_state(rng, n) * 1.7


def _backward(SV, nl, g, shard, tile_option, xs, zs, phis, psi, lam, want, passes_want, tag):
    """ovqe_adjoint_rotations on shard ``shard`` of (psi, lam), twice on the same inputs, against want = (w, psi, lam) of the reference"""
    import torch
    sl = slice(shard << nl, (shard + 1) << nl)
    w_ref, psi_ref, lam_ref = want
    with SV(nl, n_global=g, shard_index=shard) as sv:
        if tile_option is not None:
            sv.set_option("adjoint_tile_bits", tile_option)
        ws = []
        for rep in range(2):
            sv.set_state(psi[sl])
            lam_dev = torch.from_numpy(lam[sl].copy()).to("cuda:0")
            ws.append(sv.adjoint_rotations(lam_dev.data_ptr(), xs, zs, phis))
            passes, nbytes = sv.last_passes()
            if rep == 0:
                got_psi, got_lam = sv.get_state(), lam_dev.cpu().numpy()
            del lam_dev
    err = (np.abs(ws[0] - w_ref[shard]).max(), np.abs(got_psi - psi_ref[sl]).max(), np.abs(got_lam - lam_ref[sl]).max())
    print(f"{tag}: {len(xs)} rotations, passes {passes} (model {passes_want}), errors w / psi / lam {err}")
    assert max(err) < 1e-12
    assert passes == passes_want
    assert nbytes == 64 * (1 << nl) * passes
    assert np.array_equal(ws[0], ws[1])


# ---- A: backward caps ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("placement", rc.PLACEMENTS)
@pytest.mark.parametrize("name", rc.COMPLEX_BUILDERS)
@pytest.mark.parametrize("nl,g,shard,M,C", [(13, 0, 0, 11, 128), (13, 1, 1, 11, 128), (14, 0, 0, 12, 256), (14, 2, 3, 12, 256)])
def test_backward_at_the_rotation_cap(SV, nl, g, shard, M, C, name, placement):
    from tests.test_gpu_shard_gradient import _reference
    assert C == rc.adjoint_rot_cap(M)
    psi, lam = _states(nl + g, 100 * nl + g)
    xs, zs, phis = rc.build(name, C, M, nl, g, placement)
    p = rc.plan(xs, nl, M, C)
    assert len(p.segments) >= 1
    want = _reference(psi, lam, xs, zs, phis, nl, g)
    _backward(SV, nl, g, shard, M, xs, zs, phis, psi, lam, want, p.backward_passes, f"A {(nl, g, shard, M)} {name}/{placement}")


# ---- B: forward caps -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("placement", rc.PLACEMENTS)
@pytest.mark.parametrize("name", rc.COMPLEX_BUILDERS)
@pytest.mark.parametrize("tile_bits,nl,g,shard", [(10, 12, 0, 0), (11, 13, 0, 0), (12, 14, 0, 0), (11, 13, 1, 1)])
def test_forward_at_the_rotation_cap(SV, tile_bits, nl, g, shard, name, placement):
    C, M = rc.TILE_ROT_CAP, tile_bits
    psi, _ = _states(nl + g, 200 * nl + g)
    xs, zs, phis = rc.build(name, C, M, nl, g, placement)
    p = rc.plan(xs, nl, M, C)
    ref = psi
    for x, z, phi in zip(xs, zs, phis):
        ref = masks.rotate(ref, x, z, phi)
    sl = slice(shard << nl, (shard + 1) << nl)
    with SV(nl, n_global=g, shard_index=shard) as sv:
        sv.set_option("tile_bits", tile_bits)
        sv.set_state(psi[sl])
        sv.apply_pauli_rotations(xs, zs, phis)
        passes, nbytes = sv.last_passes()
        got = sv.get_state()
    err = np.abs(got - ref[sl]).max()
    print(f"B {(tile_bits, nl, g, shard)} {name}/{placement}: {len(xs)} rotations, passes {passes} (model {p.forward_passes}), error {err}")
    assert err < 1e-12
    assert passes == p.forward_passes
    assert nbytes == 32 * (1 << nl) * passes


@pytest.mark.parametrize("placement", rc.PLACEMENTS)
@pytest.mark.parametrize("name", rc.REAL_BUILDERS)
@pytest.mark.parametrize("tile_bits,nl", [(10, 13), (11, 14), (12, 15)])
def test_forward_at_the_rotation_cap_on_real_amplitudes(SV, tile_bits, nl, name, placement):
    """option "real_state" on an adopted buffer of 2^nl doubles: tiles of 2^(tile_bits + 1) amplitudes"""
    import torch
    C, M = rc.TILE_ROT_CAP, tile_bits + 1
    rng = np.random.default_rng(300 * nl)
    start = rng.normal(size=1 << nl)
    start /= np.linalg.norm(start)
    xs, zs, phis = rc.build(name, C, M, nl, 0, placement, real=True)
    p = rc.plan(xs, nl, M, C)
    ref = start.astype(complex)
    for x, z, phi in zip(xs, zs, phis):
        ref = masks.rotate(ref, x, z, phi)
    assert np.abs(ref.imag).max() < 1e-15
    buf = torch.from_numpy(start.copy()).to("cuda:0")
    with SV(nl) as sv:
        sv.adopt_state(buf.data_ptr())
        sv.set_option("real_state", 1)
        sv.set_option("tile_bits", tile_bits)
        sv.apply_pauli_rotations(xs, zs, phis)
        passes, nbytes = sv.last_passes()
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        sv.set_option("real_state", 0)
    err = np.abs(got - ref.real).max()
    print(f"B real {(tile_bits, nl)} {name}/{placement}: {len(xs)} rotations, passes {passes} (model {p.forward_passes}), error {err}")
    assert err < 1e-12
    assert passes == p.forward_passes
    assert nbytes == 16 * (1 << nl) * passes


# ---- C: one workgroup, several tiles ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,g,shard", [(11, 0, 0), (12, 0, 0), (11, 1, 1)])
def test_backward_workgroups_walk_several_tiles(SV, M, g, shard):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    grid = cus * (2 if M == 11 else 1)                      # adjoint_tile_grid (csrc/tile_host.inc)
    nl = M + 1 + math.ceil(math.log2(grid))
    assert (1 << (nl - M)) >= 2 * grid
    psi, lam = _states(nl + g, 400 + 10 * M + g)
    xs, zs, phis = rc.multi_tile_list(M, nl, g)
    p = rc.plan(xs, nl, M, rc.adjoint_rot_cap(M))
    assert len(p.segments) == 3 and p.backward_passes == 4
    want = rc.adjoint_reference_c(psi, lam, xs, zs, phis, nl, g)
    _backward(SV, nl, g, shard, M, xs, zs, phis, psi, lam, want, 4, f"C {(nl, g, shard, M)} grid {grid}")


# ---- D: the non-temporal instantiations -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("real", [False, True])
def test_forward_production_instantiation_on_sampled_fibres(SV, real):
    import torch
    nl, seed = 25, 20250227 + int(real)
    xs, zs, phis = rc.production_forward_list(real)
    p = rc.plan(xs, nl, 13 if real else 12, rc.TILE_ROT_CAP)
    assert p.forward_passes == 3 and len(p.segments) == 2
    rng = np.random.default_rng(2500 + int(real))
    samples = [0, 1, (1 << nl) - 1, 1 << (nl - 1)] + [int(v) for v in rng.integers(0, 1 << nl, 28)]
    with SV(nl) as sv:
        if real:
            sv.set_option("real_state", 1)                  # the buffer of 2^25 complex numbers holds the 2^25 doubles
        scale = sv.randomize(seed)
        sv.apply_pauli_rotations(xs, zs, phis)
        passes, nbytes = sv.last_passes()
        worst, top = 0.0, 0.0
        for i in samples:
            G, want = rc.fibre_reference(seed, scale, i, xs, zs, phis, real)
            if real:                                        # doubles 2k, 2k + 1 are read as one complex number
                pairs = sv.get_amplitudes(G >> np.uint64(1))
                got = np.where(G & np.uint64(1), pairs.imag, pairs.real)
                assert np.abs(want.imag).max() < 1e-18
            else:
                got = sv.get_amplitudes(G)
            worst, top = max(worst, np.abs(got - want).max()), max(top, np.abs(want).max())
        if real:
            sv.set_option("real_state", 0)
    torch.cuda.empty_cache()
    bound = 8 * len(xs) * np.finfo(float).eps * top
    print(f"D forward real {real}: {len(xs)} rotations, passes {passes}, error {worst} (bound {bound}) on {len(samples)} fibres of 2^14")
    assert worst < bound
    assert passes == 3
    assert nbytes == (16 if real else 32) * (1 << nl) * passes


def test_backward_production_instantiation_against_c_oracle(SV):
    import torch
    nl = 25
    xs, zs, phis = rc.production_backward_list()
    p = rc.plan(xs, nl, 12, rc.adjoint_rot_cap(12))
    assert len(p.segments) == 2 and p.backward_passes == 2
    sv, sv2 = SV(nl), SV(nl)
    try:
        sv.randomize(20250227)                              # |psi| = 1
        sv2.randomize(777)
        sv2.vec_scale(sv2.state_ptr(), 1.7)                 # |lambda| = 1.7
        psi, lam = sv.get_state(), sv2.get_state()
        assert abs(sv2.norm2() - 1.7 ** 2) < 1e-10
        w = sv.adjoint_rotations(sv2.state_ptr(), xs, zs, phis)
        passes, nbytes = sv.last_passes()
        got_psi, got_lam = sv.get_state(), sv2.get_state()
    finally:
        sv.close()
        sv2.close()
        torch.cuda.empty_cache()
    w_ref, psi_ref, lam_ref = rc.adjoint_reference_c(psi, lam, xs, zs, phis, nl, 0)
    err = (np.abs(w - w_ref[0]).max(), np.abs(got_psi - psi_ref).max(), np.abs(got_lam - lam_ref).max())
    print(f"D backward: passes {passes}, errors w / psi / lam {err}")
    assert max(err) < 1e-12
    assert passes == 2
    assert nbytes == 64 * (1 << nl) * passes
