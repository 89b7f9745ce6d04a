"""The wave sums behind the contraction of the batched sparse kernels (sv_wave_reduce.hpp: v_permlane32_swap, v_permlane16_swap and
DPP row operations, the eight states of a workgroup reduced transposed) against the __shfl_down sums they replace, which the
testing build keeps as "sparse_dbg" = 5: the networks add the same two operands at every level of the same tree, so EVERY energy
must keep EVERY bit.  A wrong assumption about which lanes an exchange instruction moves shows here, on the device — the host
check (tests/test_wave_reduce.py) can only hold the networks against the semantics they assume.

Programs: LiH and H2O (STO-3G, UCCSD: the two instances of k_sparse_vqe_rows_shared), and the designed programs of 64 and 384 basis
states of tests/test_gpu_sparse_contraction.py ("split_row": rows over several pieces) — the smallest supports that take each
instance.  Batches: 2048, the smallest that selects the workgroup geometry, and 2053, whose last work item holds 5 of 8
evaluations.  Angles of both signs.  The same comparison runs on the per-wave geometry k_sparse_vqe_rows<2> ("sparse_shared" = 0:
the single-value network), and the energies stay within the bound of tests/test_gpu_sparse.py of the C oracle."""
import numpy as np
import pytest

from tests.test_gpu_sparse import _thetas_with_nan_tail, h2o, testing_lib  # noqa: F401
from tests.test_gpu_sparse_contraction import _build
from tests.test_gpu_sparse_shared import H2O_GEOMETRY, LIH_GEOMETRY, T, _sample_shared, lih  # noqa: F401

pytestmark = pytest.mark.gpu

BATCHES = (T, T + 5)


def _bits_0_against_5(case, want, seed):
    from openvqe_amd.backend import Statevector
    with Statevector(case.n) as sv:
        sv.set_hamiltonian(case.H)
        case.program(sv)
        for B in BATCHES:
            th = _thetas_with_nan_tail(np.random.default_rng(seed + B), B, case.K)[:B]
            assert (th < 0).any() and (th > 0).any()
            idx = _sample_shared(B)
            ref = case.oracle(th[idx])   # once per batch: both geometries are held against it
            for shared, geometry in ((1, want), (0, "per_wave")):
                sv.set_option("sparse_shared", shared)
                before = set(sv.sparse_geometries())
                sv.set_option("sparse_dbg", 0)
                e0 = sv.energy_batch(th)
                sv.set_option("sparse_dbg", 5)
                e5 = sv.energy_batch(th)
                sv.set_option("sparse_dbg", 0)
                assert sv.sparse_forms() == {"rows2"}
                assert sv.sparse_geometries() == before | {geometry}
                assert e0.shape == (B,) and np.isfinite(e0).all()
                differ = int(np.count_nonzero(e0.view(np.int64) != e5.view(np.int64)))
                print(f"B = {B}, {geometry}: {differ} of {B} energies differ in their bits between sparse_dbg 0 and 5")
                assert differ == 0
                err = np.abs(e0[idx] - ref).max()
                print(f"    max |E - oracle| on {idx.size} samples = {err:.3e} (bound {1e-11 * case.scale:.3e})")
                assert err < 1e-11 * case.scale


def test_lih_instance_keeps_every_bit(testing_lib, lih):
    _bits_0_against_5(lih, LIH_GEOMETRY, 31)


def test_h2o_instance_keeps_every_bit(testing_lib, h2o):
    _bits_0_against_5(h2o, H2O_GEOMETRY, 37)


@pytest.mark.parametrize("m, want", [(64, LIH_GEOMETRY), (384, H2O_GEOMETRY)])
def test_designed_supports_keep_every_bit(testing_lib, m, want):
    case, geometry, _, _ = _build(m, "split_row")
    assert geometry == want
    _bits_0_against_5(case, want, m)
