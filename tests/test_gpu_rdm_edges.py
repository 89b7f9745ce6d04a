"""GPU tests of the branches ovqe_rdm (csrc/rdm_host.inc run_rdm, sv_rdm_host.hpp plan, the kernels of sv_rdm.hpp) takes on large
states, each against the vectorised determinant oracle of tests/rdm_cases.py (vec_rdm, pinned to the two other oracles in
tests/test_rdm_host.py).  Every case proves from rdm_info() and the compute-unit count of the device at hand that it reached the
branch it is named for and fails with the numbers where it did not ("Which branch of the density matrices is
asserted where").  Only the option "rdm_workspace_mb" is set.

Common to all cases (_measure): max |diff| to the oracle within TOL, the result Hermitian to the bit, the row count equal to the
oracle's, the non-zero count, the real / complex form, and the same bits from a second call."""
import time

import numpy as np
import pytest

from tests import rdm_cases
from tests.test_gpu_rdm import TOL

pytestmark = pytest.mark.gpu

GRAM_BLOCK = 64            # columns of a block of the Gram matrix
TILE_BYTES = 16384         # one staged row tile of one column block
CENSUS_BLOCKS_MAX = 1024   # k_rdm_census: at most this many workgroups of four waves, one bitmap word per wave and trip
ROWS_BLOCKS_PER_CU = 16    # k_rdm_rows: at most this many workgroups of 256 elements per compute unit
TIMED_CHUNKS_MAX = 64      # per-kernel event times are kept up to this many row chunks


@pytest.fixture(scope="module")
def SV(gpu_lib):
    from openvqe_amd.backend import Statevector
    return Statevector


@pytest.fixture(scope="module")
def cus(gpu_lib):
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _width(n, order):
    return n if order == 1 else n * (n - 1) // 2


def _wpad(n, order):
    return -(-_width(n, order) // GRAM_BLOCK) * GRAM_BLOCK


def _tile_rows(real):
    return TILE_BYTES // (GRAM_BLOCK * (8 if real else 16))


def _reached(ok, what, **numbers):
    if not ok:
        pytest.fail(f"{what}: not reached on this device: " + ", ".join(f"{k}={v}" for k, v in numbers.items()))


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _call(sv, order):
    return sv.rdm1() if order == 1 else sv.rdm2(packed=True)


def _dense(n, idx, amps):
    psi = np.zeros(1 << n, np.complex128)
    psi[idx] = amps
    return psi


def _single_moves(idx, det):
    """which of `idx` are `det` with one orbital moved: they differ in two bits, one occupied on each side"""
    x = idx ^ det
    low = x & -x                                                       # lowest set bit; exactly two bits: the rest is a power of two
    rest = x ^ low
    two = (rest != 0) & ((rest & (rest - 1)) == 0)
    return two & ((idx & x) != 0) & ((det & x) != 0) & ((idx & x) != x) & ((det & x) != x)


def _measure(sv, label, n, idx, amps, real, orders=(1, 2), oracle=None):
    """the assertions every case shares -> {order: (result, rdm_info of the call)}"""
    out = {}
    for order in orders:
        t0 = time.perf_counter()
        got = _call(sv, order)
        info = sv.rdm_info()
        again = _call(sv, order)
        t1 = time.perf_counter()
        want, rows = oracle[order] if oracle else rdm_cases.vec_rdm(idx, amps, n, order)
        t2 = time.perf_counter()
        err = np.abs(got - want).max()
        print(f"{label} order={order} max|diff|={err:.3e} info={info} two calls {t1 - t0:.3f} s, oracle {t2 - t1:.3f} s")
        assert got.shape == want.shape == (_width(n, order),) * 2
        assert err <= TOL
        assert np.abs(got.real - want.real).max() <= TOL and np.abs(got.imag - want.imag).max() <= TOL
        assert np.array_equal(got, got.conj().T)                       # Hermitian to the bit
        assert info["rows"] == rows
        assert info["nonzeros"] == np.count_nonzero(amps)
        assert info["real"] == (1 if real else 0)
        if real:
            assert np.abs(got.imag).max() == 0.0
        assert np.array_equal(_bits(got), _bits(again))                # the same bits from call to call
        W = _width(n, order)
        assert info["block_pairs"] == -(-W // GRAM_BLOCK) * (-(-W // GRAM_BLOCK) + 1) // 2
        out[order] = (got, info)
    return out


# ---- A, B: dense states of 14 qubits ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def psi14():
    rng = np.random.default_rng(20250314)
    psi = rng.normal(size=1 << 14) + 1j * rng.normal(size=1 << 14)
    return psi / np.linalg.norm(psi)


def test_a_rows_kernel_wraps_its_grid_dense_complex(SV, cus, psi14):
    """A. 16 369 rows of order 2 x 128 padded columns: more 256-element workgroups than k_rdm_rows' grid cap of 16 per compute unit,
    so the grid-stride loop runs a second trip (e / wpad for e beyond one grid); and several staged tiles per slice in
    k_rdm_gram<false>"""
    n = 14
    with SV(n) as sv:
        sv.set_state(psi14)
        res = _measure(sv, "A", n, np.arange(1 << n), psi14, real=False)
        assert np.array_equal(sv.get_state(), psi14)                   # the state is only read
    info = res[2][1]
    assert info["rows"] == 16369 and info["chunks"] == 1 and info["block_pairs"] == 3
    _reached(info["rows"] * _wpad(n, 2) / 256 > ROWS_BLOCKS_PER_CU * cus, "A: second trip of k_rdm_rows",
             rows=info["rows"], wpad=_wpad(n, 2), cus=cus)
    _reached(info["rows"] > _tile_rows(False) * info["row_slices"], "A: several tiles per slice in k_rdm_gram<false>",
             rows=info["rows"], row_slices=info["row_slices"])
    assert np.abs(res[2][0].imag).max() > 1e-4                         # the imaginary parts are there to be compared


def test_b_two_tiles_per_slice_in_the_real_gram_kernel(SV, cus, psi14):
    """B. the real parts of A: 512 tiles of 32 rows in at most 256 slices, so k_rdm_gram<true> runs the second trip of its tile
    loop (with the barrier that protects the staged tile); k_rdm_rows<true> wraps as in A"""
    n = 14
    psi = psi14.real / np.linalg.norm(psi14.real)
    with SV(n) as sv:
        sv.set_state(psi)
        res = _measure(sv, "B", n, np.arange(1 << n), psi, real=True)
    info = res[2][1]
    assert info["rows"] == 16369 and info["chunks"] == 1
    _reached(info["rows"] > _tile_rows(True) * info["row_slices"], "B: two tiles per slice in k_rdm_gram<true>",
             rows=info["rows"], row_slices=info["row_slices"])
    _reached(info["rows"] * _wpad(n, 2) / 256 > ROWS_BLOCKS_PER_CU * cus, "B: second trip of k_rdm_rows<true>",
             rows=info["rows"], wpad=_wpad(n, 2), cus=cus)


# ---- C, C': sparse states of 20 qubits -----------------------------------------------------------------------------------------
class CaseC:
    n = 20

    def __init__(self, SV):
        n = self.n
        self.idx, self.amps = rdm_cases.sparse_state(n, 3000, 20)
        t0 = time.perf_counter()
        self.oracle = {order: rdm_cases.vec_rdm(self.idx, self.amps, n, order) for order in (1, 2)}
        t1 = time.perf_counter()
        self.second = rdm_cases.det_rdm(self.idx, self.amps, n, 2)      # the determinant loop once, as the pin at this size
        print(f"C oracles: vec_rdm {t1 - t0:.3f} s, det_rdm {time.perf_counter() - t1:.3f} s")
        with SV(n) as sv:
            sv.set_state(_dense(n, self.idx, self.amps))
            self.res = _measure(sv, "C", n, self.idx, self.amps, real=True, oracle=self.oracle)


@pytest.fixture(scope="module")
def case_c(SV):
    return CaseC(SV)


def test_c_census_wraps_its_grid_sparse_real(case_c, cus):
    """C. 2^14 bitmap words against a census grid of 1024 workgroups x 4 waves: four trips, cnt and im accumulated across them;
    shadow strides up to word bit 13, a scan over 16 385 counts; 131 981 rows of P = 190 in three column blocks: the rows kernel
    wraps many times and k_rdm_gram<true> stages many tiles per slice"""
    c, n = case_c, case_c.n
    assert np.abs(c.oracle[2][0] - c.second).max() < 1e-14             # the oracle against the determinant loop at size
    words = 2 ** (n - 6)
    _reached(words / 4 > CENSUS_BLOCKS_MAX, "C: second trip of k_rdm_census", words=words)
    assert words > 2048                                                # the scan, and shadow strides above word bit 11
    info = c.res[2][1]
    assert info["block_pairs"] == 6 and info["chunks"] == 1
    _reached(info["rows"] * _wpad(n, 2) / 256 > 2 * ROWS_BLOCKS_PER_CU * cus, "C: third trip of k_rdm_rows",
             rows=info["rows"], wpad=_wpad(n, 2), cus=cus)
    _reached(info["rows"] > 2 * _tile_rows(True) * info["row_slices"], "C: more than two tiles per slice",
             rows=info["rows"], row_slices=info["row_slices"])


def test_c_one_imaginary_amplitude_among_real_ones(SV, case_c):
    """C'. one amplitude of C times 1j, in a bitmap word that the census reaches on a later trip than its first: `im` carried across
    trips decides for the 16-byte form (the 8-byte form would drop the imaginary part silently).  Then the same state with every
    imaginary part -0.0: the 8-byte form, and the bits of C"""
    c, n = case_c, case_c.n
    words = 2 ** (n - 6)
    per_trip = 4 * min(CENSUS_BLOCKS_MAX, words // 4)                  # words of one trip of the census grid
    late = np.flatnonzero((c.idx >> 6) >= per_trip)
    _reached(late.size > 0, "C': an amplitude beyond the first trip of k_rdm_census", words=words, per_trip=per_trip)
    # of those, one that shares a row of order 1 with another determinant (one orbital moved): gamma gets imaginary parts too
    j = next((int(k) for k in late[late.size // 2:] if np.any(_single_moves(c.idx, int(c.idx[k])))), None)
    assert j is not None, "no determinant of a later trip has a neighbour one orbital away"
    assert (int(c.idx[j]) >> 6) // per_trip >= 1
    amps = c.amps.astype(np.complex128)
    amps[j] = complex(0.0, c.amps[j])                                  # times 1j: purely imaginary, the norm unchanged
    assert amps[j].real == 0.0 and amps[j].imag != 0.0 and np.count_nonzero(amps.imag) == 1
    with SV(n) as sv:
        sv.set_state(_dense(n, c.idx, amps))
        res = _measure(sv, "C'", n, c.idx, amps, real=False)
        for order in (1, 2):
            got, want = res[order][0], rdm_cases.vec_rdm(c.idx, amps, n, order)[0]
            assert np.abs(want.imag).max() > 0.0 and np.abs(got.imag).max() > 0.0
            assert np.abs(got.imag - want.imag).max() <= TOL
        # the same handle: back to real values, all imaginary parts -0.0 (the whole register)
        psi = np.zeros(1 << n, np.complex128)
        parts = psi.view(np.float64).reshape(-1, 2)
        parts[:, 1] = -0.0
        parts[c.idx, 0] = c.amps
        assert np.signbit(psi.imag).all() and np.array_equal(psi.real[c.idx], c.amps)
        sv.set_state(psi)
        assert np.signbit(sv.get_state().imag).all()
        back = _measure(sv, "C' (-0.0)", n, c.idx, c.amps, real=True, oracle=c.oracle)
    for order in (1, 2):
        assert np.array_equal(_bits(back[order][0]), _bits(c.res[order][0]))


# ---- D: more than 64 chunks ---------------------------------------------------------------------------------------------------------
def test_d_untimed_schedule_then_a_timed_call_on_the_same_handle(SV):
    """D. dense complex, n = 12, the smallest workspace: 4083 rows in 256 chunks of one 16-row tile, the last of 3 rows — above
    TIMED_CHUNKS_MAX the per-kernel events are not recorded.  Two column blocks (2 valid columns in the last): `+=` into the slabs of
    the off-diagonal block pair across chunks.  Then the default workspace on the same handle: the event schedule of a timed call
    after an untimed one"""
    n = 12
    rng = np.random.default_rng(20250412)
    psi = rng.normal(size=1 << n) + 1j * rng.normal(size=1 << n)
    psi /= np.linalg.norm(psi)
    idx = np.arange(1 << n)
    oracle = {order: rdm_cases.vec_rdm(idx, psi, n, order) for order in (1, 2)}
    with SV(n) as sv:
        sv.set_state(psi)
        one = _measure(sv, "D one chunk", n, idx, psi, real=False, oracle=oracle)
    assert one[2][1]["chunks"] == 1
    with SV(n) as sv:
        sv.set_state(psi)
        sv.set_option("rdm_workspace_mb", 0)
        many = _measure(sv, "D minimum workspace", n, idx, psi, real=False, oracle=oracle)
        info = many[2][1]
        assert info["rows"] == 4083 and info["block_pairs"] == 3 and info["row_slices"] == 1
        _reached(info["chunks"] > TIMED_CHUNKS_MAX, "D: untimed schedule", chunks=info["chunks"])
        assert info["chunks"] == 256 and info["gram_launches"] == 256 and info["rows"] - 255 * 16 == 3
        assert info["workspace_bytes"] == 16 * _wpad(n, 2) * 16
        assert info["rows_us"] == 0 and info["gram_us"] == 0 and info["finish_us"] == 0      # not timed
        for order in (1, 2):
            err = np.abs(many[order][0] - one[order][0]).max()
            print(f"D order={order} chunks={many[order][1]['chunks']} max|diff| to one chunk {err:.3e}")
            assert err <= 1e-13
        sv.set_option("rdm_workspace_mb", 1024)
        back = _measure(sv, "D default workspace again", n, idx, psi, real=False, oracle=oracle)
        assert np.array_equal(sv.get_state(), psi)
    for order in (1, 2):
        info = back[order][1]
        assert info["chunks"] == 1
        assert info["rows_us"] >= 0 and info["gram_us"] > 0 and info["finish_us"] >= 0 and info["list_us"] >= 0
        assert np.array_equal(_bits(back[order][0]), _bits(one[order][0]))


# ---- E: complex, two column blocks, several chunks, empty slices ------------------------------------------------------------------
def test_e_complex_chunks_with_empty_slices_in_the_last_launch(SV):
    """E. 88 random determinants with complex amplitudes at n = 13 (P = 78: two column blocks), 1 MB of workspace = chunks of 512
    rows of 128 complex: 1653 rows in 4 chunks, the last of 117 rows — 8 of the 32 slices of 16 rows, the other workgroups of the
    last launch return before they touch their slab"""
    n = 13
    idx, amps = rdm_cases.sparse_state(n, 88, 13, complex_amps=True)
    oracle = {order: rdm_cases.vec_rdm(idx, amps, n, order) for order in (1, 2)}
    psi = _dense(n, idx, amps)
    with SV(n) as sv:
        sv.set_state(psi)
        default = _measure(sv, "E default workspace", n, idx, amps, real=False, oracle=oracle)
    with SV(n) as sv:
        sv.set_state(psi)
        sv.set_option("rdm_workspace_mb", 1)
        small = _measure(sv, "E 1 MB", n, idx, amps, real=False, oracle=oracle)
    info = small[2][1]
    row_bytes = _wpad(n, 2) * 16
    chunk_rows = info["workspace_bytes"] // row_bytes
    tiles = chunk_rows // _tile_rows(False)
    slice_rows = -(-tiles // info["row_slices"]) * _tile_rows(False)
    last = info["rows"] - (info["chunks"] - 1) * chunk_rows
    assert info["workspace_bytes"] == 1 << 20 and chunk_rows == 512 and info["block_pairs"] == 3
    assert default[2][1]["chunks"] == 1 and info["gram_launches"] == info["chunks"]
    _reached(1 < info["chunks"] <= TIMED_CHUNKS_MAX, "E: several timed chunks", chunks=info["chunks"])
    _reached(0 < last <= slice_rows * (info["row_slices"] - 1), "E: an empty slice in the last launch", rows=info["rows"],
             chunks=info["chunks"], chunk_rows=chunk_rows, row_slices=info["row_slices"], slice_rows=slice_rows, last=last)
    print(f"E: last chunk {last} rows = {-(-last // slice_rows)} of {info['row_slices']} slices of {slice_rows} rows")
    for order in (1, 2):
        err = np.abs(small[order][0] - default[order][0]).max()
        print(f"E order={order} chunks={small[order][1]['chunks']} max|diff| to the default workspace {err:.3e}")
        assert err <= 1e-13


# ---- F: five column blocks --------------------------------------------------------------------------------------------------------
def test_f_five_column_blocks_at_24_qubits(SV, cus):
    """F. 2000 random determinants at n = 24: P = 276 = four blocks of 64 and one of 20 valid columns, 15 block pairs —
    block_pair / block_pair_index for nblk = 5 on the device; 138 006 rows; a census of 2^18 words in 64 trips"""
    n = 24
    idx, amps = rdm_cases.sparse_state(n, 2000, 24)
    with SV(n) as sv:
        sv.set_state(_dense(n, idx, amps))
        res = _measure(sv, "F", n, idx, amps, real=True)
    info = res[2][1]
    _reached(info["block_pairs"] == 15, "F: five column blocks", block_pairs=info["block_pairs"])
    assert _width(n, 2) == 276 and _width(n, 2) - 4 * GRAM_BLOCK == 20
    assert info["rows"] > 100000 and info["chunks"] == 1
    assert 2 ** (n - 6) / 4 > CENSUS_BLOCKS_MAX
    _reached(info["rows"] * _wpad(n, 2) / 256 > ROWS_BLOCKS_PER_CU * cus, "F: k_rdm_rows wraps", rows=info["rows"], cus=cus)
    # traces from the amplitudes and the popcounts directly.  Bound: each trace sums at most 276 elements that are sums of squares
    # adding up to <N> <= 24 resp. <N(N-1)/2> <= 276 — rounding far below the 1e-12 of test_sparse_real_state's trace checks
    occ = np.array([bin(int(i)).count("1") for i in idx], np.float64)
    w = amps * amps
    n_want, pairs_want = float(np.sum(w * occ)), float(np.sum(w * occ * (occ - 1) / 2))
    n_got, pairs_got = np.trace(res[1][0]), np.trace(res[2][0])
    print(f"F <N> {n_got.real:.15f} / {n_want:.15f}, <N(N-1)/2> {pairs_got.real:.15f} / {pairs_want:.15f}")
    assert n_got.imag == 0.0 and pairs_got.imag == 0.0
    assert abs(n_got.real - n_want) < 1e-12 and abs(pairs_got.real - pairs_want) < 1e-12


# ---- G: zero rows -------------------------------------------------------------------------------------------------------------------
def test_g_vacuum_one_particle_and_the_full_register(SV):
    """G. |0...0>: one non-zero amplitude, no row, no chunk, no Gram launch — finish over zeroed slabs.  One particle: a single 1.0
    in gamma, order 2 without rows.  All orbitals occupied: both matrices are the identity, exactly"""
    n, k = 7, 2
    one = np.array([1.0 + 0j])
    with SV(n) as sv:
        sv.init_basis(0)
        res = _measure(sv, "G vacuum", n, np.array([0]), one, real=True)
        for order in (1, 2):
            got, info = res[order]
            assert info["nonzeros"] == 1 and info["rows"] == 0 and info["chunks"] == 0 and info["gram_launches"] == 0
            assert np.array_equal(got, np.zeros_like(got))
        sv.init_basis(1 << k)
        res = _measure(sv, "G one particle", n, np.array([1 << k]), one, real=True)
        want = np.zeros((n, n), np.complex128)
        want[n - 1 - k, n - 1 - k] = 1.0                                # orbital p = index bit n-1-p
        assert np.array_equal(res[1][0], want) and res[1][1]["rows"] == 1
        assert np.array_equal(res[2][0], np.zeros_like(res[2][0])) and res[2][1]["rows"] == 0 and res[2][1]["chunks"] == 0
        sv.init_basis(2 ** n - 1)
        res = _measure(sv, "G full register", n, np.array([2 ** n - 1]), one, real=True)
        assert np.array_equal(res[1][0], np.eye(n, dtype=np.complex128)) and res[1][1]["rows"] == n
        assert np.array_equal(res[2][0], np.eye(n * (n - 1) // 2, dtype=np.complex128)) and res[2][1]["rows"] == n * (n - 1) // 2


# ---- H: one handle, many different calls --------------------------------------------------------------------------------------------
def test_h_one_handle_through_changing_states_sizes_and_workspaces(SV):
    """H. what RdmDev keeps between calls (workspace, slabs, row list, column table, events) through calls that change the element
    size, the width, the workspace option and the state: every result has the bits of the same call on a fresh handle"""
    n = 12
    rng = np.random.default_rng(20250512)
    dense = rng.normal(size=1 << n) + 1j * rng.normal(size=1 << n)
    dense /= np.linalg.norm(dense)
    sparse_a = _dense(n, *rdm_cases.sparse_state(n, 40, 121))
    sparse_b = _dense(n, *rdm_cases.sparse_state(n, 150, 122))
    steps = [(sparse_a, None, 2), (dense, None, 1), (None, 0, 2), (sparse_b, 1024, 2), (None, None, 1)]   # (new state, workspace, order)

    def fresh(psi, mb, order):
        with SV(n) as sv:
            sv.set_state(psi)
            if mb is not None:
                sv.set_option("rdm_workspace_mb", mb)
            return _call(sv, order), sv.rdm_info()

    t0 = time.perf_counter()
    with SV(n) as sv:
        psi, mb = None, None
        for step, (new_psi, new_mb, order) in enumerate(steps, 1):
            if new_psi is not None:
                psi = new_psi
                sv.set_state(psi)
            if new_mb is not None:
                mb = new_mb
                sv.set_option("rdm_workspace_mb", mb)
            got = _call(sv, order)
            info = sv.rdm_info()
            assert np.array_equal(_bits(sv.get_state()), _bits(psi))   # the state buffer is unchanged throughout
            want, want_info = fresh(psi, mb, order)
            idx = np.flatnonzero(psi)
            ref, rows = rdm_cases.vec_rdm(idx, psi[idx], n, order)
            err = np.abs(got - ref).max()
            print(f"H step {step} order={order} workspace={mb} max|diff|={err:.3e} info={info}")
            assert err <= TOL and info["rows"] == rows and np.array_equal(got, got.conj().T)
            for key in ("nonzeros", "rows", "chunks", "real", "workspace_bytes", "gram_launches", "block_pairs", "row_slices"):
                assert info[key] == want_info[key], key
            assert np.array_equal(_bits(got), _bits(want)), f"step {step}"
            if step == 3:
                assert info["chunks"] > TIMED_CHUNKS_MAX and info["real"] == 0
            if step in (1, 4, 5):
                assert info["real"] == 1 and info["chunks"] == 1
    print(f"H: {time.perf_counter() - t0:.3f} s")
