"""GPU tests of the subspace-expansion kernels AT THEIR LIMITS (k_sub_shadow, k_sub_expand<DENSE>, k_sub_sigma<DENSE, NB>, k_sub_gram,
k_sub_finish_full in csrc/sv_subspace.hpp, the plan in csrc/sv_subspace_host.hpp, the launches in csrc/subspace_host.inc): the NB = 4
instantiation of the sigma kernel with full and cut-off last column groups, Gram slices of several row tiles up to the cap of 256 slices
and with a short last slice, the grid-stride loops of the expand and sigma kernels, registers below one bitmap word with sparse states,
calls without rows, rows on which no x-group of H is live or exactly one lane of a batch is, and one handle called with changing shapes.

Every case is compared with the checker of tests/subspace_cases.py through ``compare`` — |dS_ij| <= 1e-12 a_i a_j,
|dG_ij| <= 1e-10 (||H||_1 + |constant|) a_i a_j — repeats its bits on a second call, leaves the state buffer untouched, and shows in
``subspace_info()`` that it took the path it is named for: the path figures are compared with ``subspace_cases.plan`` at the 256 CUs
of an MI355X, and the branch of each named case with its predicate in ``subspace_cases.EDGE_CASES``."""
import numpy as np
import pytest

from openvqe_amd.operators import Hamiltonian
from tests import subspace_cases as sc
from tests import util

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def SV(gpu_lib):
    from openvqe_amd.backend import Statevector
    return Statevector


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _call(sv, ops, with_h):
    if with_h:
        return sv.subspace_matrices(ops, raw=True)
    return None, sv.subspace_matrices(ops, hamiltonian=False)


def _same_bits(G, S, G2, S2):
    return np.array_equal(_bits(S), _bits(S2)) and (G is None or np.array_equal(_bits(G), _bits(G2)))


def _check(what, n, psi, ops, ham, with_h, G, S, info, name=None):
    """against the checker and the restated plan; -> (plan, rows)"""
    want_S, want_G, rows = sc.matrices(psi, n, ops, ham if with_h else None)
    sc.compare(what, S, G, want_S, want_G, n, ops, ham if with_h else None)
    p = sc.check_info_against_plan(info, rows, len(ops), with_h)
    assert info["dense"] == int(rows == 1 << n), info
    assert info["h_groups"] == (len(sc.handle_group_order(n, ham)) if with_h else 0)
    if name is not None:
        (cn, crows, cm, cwith_h), branch = sc.EDGE_CASES[name]
        assert (cn, crows, cm, cwith_h) == (n, rows, len(ops), with_h), (name, rows)
        assert branch(p), (name, p)          # the case reached the path it is named for
    return p, rows


def _run(SV, what, n, psi, ops, ham, with_h=True, name=None):
    """one fresh handle: the call, its figures, the state afterwards, the call again; -> (G, S, info, plan)"""
    with SV(n) as sv:
        sv.set_hamiltonian(ham)
        sv.set_state(psi)
        before = sv.get_state()
        G, S = _call(sv, ops, with_h)
        info = sv.subspace_info()
        after = sv.get_state()
        G2, S2 = _call(sv, ops, with_h)
    assert np.array_equal(_bits(before), _bits(np.asarray(psi, np.complex128))) and np.array_equal(_bits(before), _bits(after))
    assert _same_bits(G, S, G2, S2), what
    p, _ = _check(what, n, psi, ops, ham, with_h, G, S, info, name)
    print(f"{what}: rows {info['rows']}, slices {info['slices']} x {info['slice_rows']} rows, NB {info['sigma_blocks']} x "
          f"{info['sigma_col_groups']} groups, grids sigma {info['sigma_grid']} expand {info['expand_grid']}; "
          f"expand {info['expand_us']} us, sigma {info['sigma_us']} us, Gram {info['gram_us']} us")
    return G, S, info, p


# ---- 1. widths of the sigma and expand kernels ------------------------------------------------------------------------------------------
SPARSE_XS = [0, 0b10010110]


def _width_case(form, m):
    rng = np.random.default_rng(7000 + m)
    if form == "dense":
        n = sc.WIDTH_DENSE_N
        return n, util.random_state(rng, n), sc.random_pool(rng, n, m), util.random_hamiltonian(rng, n, 12, constant=0.375)
    n = sc.WIDTH_SPARSE_N
    psi = sc.closed_support_state(rng, n, sc.WIDTH_SPARSE_ROWS, SPARSE_XS)
    ham = sc.small_hamiltonian(rng, n, [0, SPARSE_XS[1], 1, 0b1000, 0b10010111, 0b11111111, 0b01100000])
    return n, psi, sc.pool_with_x(rng, n, m, SPARSE_XS), ham


@pytest.mark.parametrize("m", sc.WIDTHS)
@pytest.mark.parametrize("form", ["dense", "sparse"])
def test_sigma_and_expand_widths(SV, form, m):
    """m = 192 is the last pool of NB = 2 (two column groups), 193 the first of NB = 4; 256 fills its four blocks, 257 has ONE live column
    in the only block of its second column group (blk0 + b < nb cuts three blocks off), 320 fills that block, 321 opens a sixth block;
    mb = 192, 256, 320, 384 are the divisors of k_sub_expand.  Dense on 7 qubits; sparse on 8 with 42 rows, off the row tile of 4."""
    n, psi, ops, ham = _width_case(form, m)
    _, _, info, _ = _run(SV, f"width {form} m={m}", n, psi, ops, ham, name=f"width {form} m={m}")
    assert info["sigma_blocks"] == (4 if m >= 193 else 2)
    assert info["sigma_col_groups"] == (2 if m >= 257 or m == 192 else 1)
    assert info["rows"] % 4 == (0 if form == "dense" else 2)


@pytest.mark.parametrize("form", ["dense", "sparse"])
def test_overlap_alone_at_257_operators_has_the_bits_of_the_full_call(SV, form):
    n, psi, ops, ham = _width_case(form, 257)
    _, S_full, _, _ = _run(SV, f"width {form} m=257 (for S alone)", n, psi, ops, ham, name=f"width {form} m=257")
    _, S, info, _ = _run(SV, f"width {form} m=257 S alone", n, psi, ops, ham, with_h=False, name=f"width {form} m=257 S only")
    assert info["sigma_blocks"] == 0 and info["sigma_launches"] == 0 and info["sigma_grid"] == 0
    assert np.array_equal(_bits(S), _bits(S_full))


# ---- 2. Gram slices -----------------------------------------------------------------------------------------------------------------------
def test_gram_slice_of_two_row_tiles(SV):
    """9 qubits dense, m = 257: 40 block pairs, 26 slices wanted of 32 tiles -> 16 slices of 32 rows: k_sub_gram stages two tiles"""
    n, m = 9, 257
    rng = np.random.default_rng(92)
    _, _, info, _ = _run(SV, "gram two tiles", n, util.random_state(rng, n), sc.random_pool(rng, n, m),
                         util.random_hamiltonian(rng, n, 12, constant=0.375), name="gram two tiles")
    assert info["slice_rows"] > 16 and info["block_pairs"] == 40


def test_gram_slices_at_their_cap(SV):
    """13 qubits dense, m = 2: one block, 512 tiles and 512 slices wanted, GRAM_MAX_SLICES = 256 holds them at two tiles each"""
    n = 13
    rng = np.random.default_rng(132)
    _, _, info, _ = _run(SV, "gram slice cap", n, util.random_state(rng, n), sc.random_pool(rng, n, 2),
                         util.random_hamiltonian(rng, n, 10, constant=0.375), name="gram slice cap")
    assert info["slices"] == 256 and info["slice_rows"] == 32


@pytest.mark.parametrize("name,n,rows,xs,slices,slice_rows", [
    ("gram short last slice", 13, 4101, [0], 129, 32),        # 257 tiles: the last slice holds 5 rows, one partial tile
    ("gram rows % 16 == 1", 13, 4113, [0], 129, 32),          # the last slice holds 17 rows: a full tile, then a tile of one row
    ("gram rows == 16 slices", 10, 592, [0, 0b1100000011, 0b0011000000, 0b101, 0b10], 37, 16)])   # every tile full, no slice short
def test_gram_slices_of_sparse_row_sets(SV, name, n, rows, xs, slices, slice_rows):
    rng = np.random.default_rng(rows)
    psi = sc.closed_support_state(rng, n, rows, xs)
    ops = sc.pool_with_x(rng, n, 3, xs)
    ham = sc.small_hamiltonian(rng, n, [0, 1, 0b11, 1 << (n - 1), (1 << n) - 1, 0b0011000000, 0b1010101])
    _, _, info, _ = _run(SV, name, n, psi, ops, ham, name=name)
    assert (info["rows"], info["slices"], info["slice_rows"], info["dense"]) == (rows, slices, slice_rows, 0)


# ---- 3. grid strides ------------------------------------------------------------------------------------------------------------------------
def test_grid_strides_on_a_dense_register_of_16_qubits(SV):
    """65 536 rows, m = 3: 16 384 row tiles for at most 8192 workgroups of k_sub_sigma, 2^22 store elements for at most 4096 workgroups
    of k_sub_expand: both loops take a second pass.  The store is 128 MiB."""
    n = 16
    rng = np.random.default_rng(16)
    _, _, info, _ = _run(SV, "stride dense", n, util.random_state(rng, n), sc.random_pool(rng, n, 3),
                         util.random_hamiltonian(rng, n, 8, constant=0.375), name="stride dense")
    assert info["sigma_grid"] * 4 < info["rows"] and info["expand_grid"] * 256 < info["rows"] * 64
    assert info["store_bytes"] == 128 << 20


def test_grid_strides_on_a_sparse_state_of_40000_rows(SV):
    """the same register, 40 000 rows in 5000 cosets of three x masks: the non-dense kernels stride, and the row lookup of the sigma
    kernel runs across 1024 bitmap words; four x-groups of H stay inside R, three leave it"""
    n = 16
    xs = [0, 0x8001, 0x0180, 0x4002]
    rng = np.random.default_rng(40000)
    psi = sc.closed_support_state(rng, n, 40000, xs)
    ham = sc.small_hamiltonian(rng, n, [0, 0x8001, 0x8001 ^ 0x0180, 0x4002 ^ 0x0180 ^ 0x8001, 0x0010, 0x1234, 0xffff])
    _, _, info, _ = _run(SV, "stride sparse", n, psi, sc.pool_with_x(rng, n, 3, xs), ham, name="stride sparse")
    assert info["dense"] == 0 and info["rows"] == 40000
    assert info["sigma_grid"] * 4 < info["rows"] and info["expand_grid"] * 256 < info["rows"] * 64


# ---- 4. a register below one bitmap word, sparse states ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 5])
@pytest.mark.parametrize("support", ["one", "two", "all but one"])
@pytest.mark.parametrize("n", [3, 4, 5])
def test_sparse_states_below_one_bitmap_word(SV, n, support, m):
    """xor_word and row_position on a partial word, the non-dense kernels on 3 .. 5 qubits: supports of 1, 2 and 2^n - 1 indices, the
    pool's x masks 1, 2^n - 1 and a middle bit (m = 1: the identity alone, R is the support)"""
    rng = np.random.default_rng(100 * n + 10 * m + len(support))
    size = {"one": 1, "two": 2, "all but one": (1 << n) - 1}[support]
    psi = np.zeros(1 << n, np.complex128)
    where = rng.choice(1 << n, size, replace=False)
    psi[where] = rng.normal(size=size) + 1j * rng.normal(size=size)
    psi /= np.linalg.norm(psi)
    ops = sc.pool_with_x(rng, n, m, [1, (1 << n) - 1, 1 << (n // 2)] if m > 1 else [0])
    ham = util.random_hamiltonian(rng, n, 6, constant=0.375)
    _, _, info, _ = _run(SV, f"partial word n={n} support {size} m={m}", n, psi, ops, ham)
    rows = sc.expected_rows(psi, n, ops)
    assert info["rows"] == rows and info["dense"] == int(rows == 1 << n)
    if m == 1:
        assert rows == size and info["dense"] == 0
    if support != "all but one":
        assert info["dense"] == 0 and rows < (1 << n)


# ---- 5. no rows ---------------------------------------------------------------------------------------------------------------------------
def _assert_no_rows(G, S, info):
    assert np.all(S == 0) and np.all(G == 0)          # (values: the mirrored triangle of S holds -0.0 in its imaginary parts)
    for key in ("rows", "expand_launches", "sigma_launches", "sigma_blocks", "sigma_grid", "expand_grid"):
        assert info[key] == 0, (key, info)
    assert info["gram_launches"] == 1 and info["slices"] == 1


def test_the_zero_state_gives_zero_matrices_and_the_next_call_is_correct(SV):
    n = 6
    rng = np.random.default_rng(60)
    ops, ham = sc.random_pool(rng, n, 5), util.random_hamiltonian(rng, n, 10, constant=0.375)
    zero, psi = np.zeros(1 << n, np.complex128), util.random_state(rng, n)
    with SV(n) as sv:
        sv.set_hamiltonian(ham)
        sv.set_state(psi)
        sv.subspace_matrices(ops)                                     # (a call with rows first: the buffers hold its figures)
        sv.set_state(zero)
        G, S = sv.subspace_matrices(ops, raw=True)
        info = sv.subspace_info()
        G2, S2 = sv.subspace_matrices(ops, raw=True)
        assert np.all(_bits(sv.get_state()) == 0)
        sv.set_state(psi)
        Gn, Sn = sv.subspace_matrices(ops, raw=True)
        info_n = sv.subspace_info()
    _assert_no_rows(G, S, info)
    assert _same_bits(G, S, G2, S2)
    _check("zero state", n, zero, ops, ham, True, G, S, info, name="zero rows")
    _check("after the zero state", n, psi, ops, ham, True, Gn, Sn, info_n)


def test_a_pool_of_empty_operators_gives_zero_matrices_and_the_next_call_is_correct(SV):
    n = 6
    rng = np.random.default_rng(61)
    empty = [Hamiltonian(n, [], 0.0) for _ in range(3)]
    ops, ham = sc.random_pool(rng, n, 5), util.random_hamiltonian(rng, n, 10, constant=0.375)
    psi = util.random_state(rng, n)
    with SV(n) as sv:
        sv.set_hamiltonian(ham)
        sv.set_state(psi)
        G, S = sv.subspace_matrices(empty, raw=True)
        info = sv.subspace_info()
        G2, S2 = sv.subspace_matrices(empty, raw=True)
        after = sv.get_state()
        Gn, Sn = sv.subspace_matrices(ops, raw=True)
        info_n = sv.subspace_info()
    _assert_no_rows(G, S, info)
    assert info["distinct_x"] == 0 and info["m"] == 3
    assert _same_bits(G, S, G2, S2) and np.array_equal(_bits(after), _bits(psi))
    _check("empty pool", n, psi, empty, ham, True, G, S, info)
    _check("after the empty pool", n, psi, ops, ham, True, Gn, Sn, info_n)


# ---- 6. dead and lone x-groups ------------------------------------------------------------------------------------------------------------
AGREEING_XS = [0, 0b110000, 0b001111, 0b111100]       # both bits of every pair (0, 1), (2, 3), (4, 5) or neither


@pytest.mark.parametrize("ulp", [False, True])
def test_cancelling_groups_on_a_dense_state(SV, ulp):
    """1/2 (XX + YY) on the pairs (0, 1), (2, 3), (4, 5): on a dense state every group is dead on half of the rows and every row has a
    dead group; with ``ulp`` the two coefficients differ by one ulp and the residue is what group_coeff_snap removes"""
    n = 6
    rng = np.random.default_rng(66 + ulp)
    _run(SV, f"cancelling dense ulp={ulp}", n, util.random_state(rng, n), sc.random_pool(rng, n, 5), sc.cancelling_hamiltonian(n, ulp=ulp))


@pytest.mark.parametrize("ulp", [False, True])
def test_rows_without_a_live_group_give_the_constant_times_phi(SV, ulp):
    """a state on the 8 indices where the bits of every pair agree, a pool that keeps them agreeing: every x-group's coefficient is zero
    (``ulp``: snaps to zero) on every row, ``live`` is false in all lanes, and sigma = constant * phi exactly.  The constant is a power of
    two, so every product and sum of Phi^H Sigma is that of Phi^H Phi scaled: G = constant * S to the bit on the upper triangle, which
    is where S is computed (the diagonal's imaginary part, a rounding residue in G, is set to zero in S)."""
    n, constant = 6, 0.25
    rng = np.random.default_rng(68 + ulp)
    where = sc.agreeing_indices(n)
    assert where.shape[0] == 8
    psi = np.zeros(1 << n, np.complex128)
    psi[where] = rng.normal(size=8) + 1j * rng.normal(size=8)
    psi /= np.linalg.norm(psi)
    ops = sc.pool_with_x(rng, n, 5, AGREEING_XS)
    G, S, info, _ = _run(SV, f"no live group ulp={ulp}", n, psi, ops, sc.cancelling_hamiltonian(n, constant, ulp=ulp))
    assert info["rows"] == 8 and info["h_groups"] == 3 and info["dense"] == 0
    upper = np.triu_indices(5)
    strict = np.triu_indices(5, 1)
    assert np.array_equal(_bits(G.real[upper]), _bits(constant * S.real[upper]))
    assert np.array_equal(_bits(G.imag[strict]), _bits(constant * S.imag[strict]))


@pytest.mark.parametrize("ngroups,which", [(65, 0), (65, 63), (65, 64), (128, 0), (128, 63), (128, 64), (128, 127)])
def test_one_live_lane_in_a_batch_of_groups(SV, ngroups, which):
    """65 and 128 x-groups: on two of the three rows only the group at position ``which`` of the handle's list has its partner inside
    R — lane 0 or lane 63 of the first batch, lane 0 or lane 63 of the second — and on the third row none has"""
    n = 9
    ham, psi, (a, b, c) = sc.one_live_group(n, ngroups, which)
    ops = sc.pool_with_x(np.random.default_rng(which), n, 4, [0])
    assert sc.live_groups(n, ham, (a, b, c), a) == [which] and sc.live_groups(n, ham, (a, b, c), c) == []
    G, _, info, _ = _run(SV, f"one live group {which} of {ngroups}", n, psi, ops, ham)
    assert info["rows"] == 3 and info["h_groups"] == ngroups
    # the live group carries weight: without it G would miss the bound by orders of magnitude
    x = which + 1
    coupling = abs(sc.group_coefficient(n, ham, x, b) * np.conj(psi[a]) * psi[b])
    assert coupling > 1e4 * sc.g_bound(n, ops, ham)[0, 0]


# ---- 7. one handle, many shapes ---------------------------------------------------------------------------------------------------------------
def test_one_handle_called_with_changing_shapes(SV):
    """dense m = 257 with H | sparse (30 rows) m = 3 with H | the same, S only | dense m = 65 S only | dense m = 65 with H | the zero
    state | dense m = 257 again: wpad, the row list, the store and the slabs change from call to call (and k_rdm_list is skipped when
    dense); every step equals the checker and the bits of the same call on a fresh handle, and the last step the first"""
    n = 10
    rng = np.random.default_rng(1010)
    sparse_xs = [0, 0b1000000001]
    dense_psi = util.random_state(rng, n)
    sparse_psi = sc.closed_support_state(rng, n, 30, sparse_xs)
    ham = util.random_hamiltonian(rng, n, 12, constant=0.375)
    pool257, pool65, pool3 = sc.random_pool(rng, n, 257), sc.random_pool(rng, n, 65), sc.pool_with_x(rng, n, 3, sparse_xs)
    zero = np.zeros(1 << n, np.complex128)
    steps = [("handle dense m=257", dense_psi, pool257, True), ("handle sparse m=3", sparse_psi, pool3, True),
             ("handle sparse m=3 S only", sparse_psi, pool3, False), ("handle dense m=65 S only", dense_psi, pool65, False),
             ("handle dense m=65", dense_psi, pool65, True), (None, zero, pool65, True), ("handle dense m=257", dense_psi, pool257, True)]
    got = []
    with SV(n) as sv:
        sv.set_hamiltonian(ham)
        for name, psi, ops, with_h in steps:
            sv.set_state(psi)
            G, S = _call(sv, ops, with_h)
            got.append((G, S, sv.subspace_info(), sv.get_state()))
    for k, ((name, psi, ops, with_h), (G, S, info, after)) in enumerate(zip(steps, got)):
        what = f"step {k + 1} ({name or 'zero state'})"
        assert np.array_equal(_bits(after), _bits(psi)), what
        _check(what, n, psi, ops, ham, with_h, G, S, info, name)
        with SV(n) as fresh:
            fresh.set_hamiltonian(ham)
            fresh.set_state(psi)
            Gf, Sf = _call(fresh, ops, with_h)
            info_f = fresh.subspace_info()
        assert _same_bits(G, S, Gf, Sf), what
        path = ("rows", "dense", "store_bytes", "slices", "slice_rows", "sigma_blocks", "sigma_col_groups", "sigma_grid", "expand_grid")
        assert {key: info[key] for key in path} == {key: info_f[key] for key in path}, what
    assert got[5][2]["rows"] == 0 and np.all(got[5][1] == 0) and np.all(got[5][0] == 0)
    assert _same_bits(got[0][0], got[0][1], got[6][0], got[6][1])
