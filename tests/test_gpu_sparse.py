"""The support-compacted path (openvqe_amd/csrc/sparse_host.inc, kernels in sv_sparse.hpp) form by form, at its boundaries, against
the C oracle (oracle/cref.py) and the adjoint gradient of oracle/masks.py.

Every test names the kernel form it means to reach and asserts through ``Statevector.sparse_forms()`` that it did, so that a change
of the thresholds cannot move a test off its target quietly.  Batches: the oracle sample holds the first two, the middle one, both
sides of every 8192-work wrap of the grid and the last two evaluations; every other energy is compared with a second form of the
same batch.  Supports are designed to an exact size (tests/util.py: cascade_geometry, pattern_excitation, support_closure)."""
import numpy as np
import pytest

from openvqe_amd.operators import Hamiltonian, Term, pack_terms
from oracle import cref, masks
from tests.util import cascade_geometry, compile_generators, pattern_excitation, support_closure, y_rotation

pytestmark = pytest.mark.gpu

GRID = 8192          # run_sparse: grid = min(nwork, 256 * 32)


@pytest.fixture
def testing_lib(gpu_lib, monkeypatch):
    """the OVQE_TESTING build of the same source ("sparse_spw", "sparse_rows", "sparse_wg" exist only there)"""
    from openvqe_amd import _lib
    monkeypatch.setattr(_lib, "LIB_PATH", _lib.TESTING_LIB_PATH)
    monkeypatch.setattr(_lib, "_lib", None)
    return _lib.lib()


class Case:
    """a rotation program (index-bit masks) and a real Hamiltonian, with the oracle's answers"""

    def __init__(self, n, hf, rx, rz, rc, rp, K, H):
        self.n, self.hf, self.K, self.H = n, int(hf), int(K), H
        self.rx, self.rz, self.rc, self.rp = rx, rz, rc, rp
        hx, hz, hc = pack_terms(n, H.terms)
        self.hx, self.hz, self.hc = hx, hz, np.ascontiguousarray(hc.real)
        self.const = float(H.constant_coeff)
        self.scale = max(1.0, float(np.abs(self.hc).sum()))

    def program(self, sv):
        sv.set_rotation_program(self.rx, self.rz, self.rc, self.rp, self.K, self.hf)

    def oracle(self, thetas):
        return cref.ucc_energy_batch(self.n, self.hf, self.rx, self.rz, self.rc, self.rp, np.asarray(thetas), self.hx, self.hz,
                                     self.hc, self.const)

    def oracle_gradient(self, theta):
        return masks.ucc_energy_gradient(self.n, self.hf, self.rx, self.rz, self.rc, self.rp, theta, self.hx, self.hz, self.hc,
                                         self.const)


def _mask_term(n, x, z, c):
    op, qs = "", []
    for q in range(n):
        b = n - 1 - q
        xb, zb = (x >> b) & 1, (z >> b) & 1
        if xb or zb:
            op += "Y" if xb and zb else ("X" if xb else "Z")
            qs.append(q)
    return Term(float(c), op, qs)


def _hamiltonian(rng, n, xmasks, nz=12):
    """diagonal Z strings plus strings of even Y count on the x masks of the program (real, with entries inside the support)"""
    terms, seen = [], set()
    for _ in range(nz):
        z = int(rng.integers(1, 1 << n))
        if (0, z) not in seen:
            seen.add((0, z))
            terms.append(_mask_term(n, 0, z, rng.normal()))
    for x in sorted(set(int(v) for v in xmasks))[:24]:
        bits = [b for b in range(n) if (x >> b) & 1]
        for _ in range(2):
            ys = [b for b in bits if rng.random() < 0.5]
            if len(ys) % 2:
                ys = ys[1:]
            z = sum(1 << b for b in ys) | (int(rng.integers(0, 1 << n)) & ~x & int(rng.integers(0, 1 << n)))
            if (x, z) not in seen:
                seen.add((x, z))
                terms.append(_mask_term(n, x, z, rng.normal()))
    return Hamiltonian(n, terms, float(rng.normal()))


def _designed(n, hf, gens, K, seed):
    rx, rz, rc, rp = compile_generators(gens)
    return Case(n, hf, rx, rz, rc, rp, K, _hamiltonian(np.random.default_rng(seed), n, rx))


def _sample(B):
    """oracle sample: first two, middle, both sides of every 8192-work wrap (for one and two evaluations per work item), last two"""
    idx = {0, 1, B // 2, B - 2, B - 1}
    for spw in (1, 2):
        for w in range(GRID, (B + spw - 1) // spw + 1, GRID):
            idx.update({w * spw - 1, w * spw, w * spw + spw - 1})
    return np.array(sorted(i for i in idx if 0 <= i < B))


def _second_form(sv, th):
    """the same energies through the per-wave / per-workgroup forms: chunks of 512 rows (a chunk shorter than 257 rows is padded by
    repeating itself, so that it takes the staged form too)"""
    out = []
    for c0 in range(0, th.shape[0], 512):
        c = th[c0:c0 + 512]
        reps = -(-257 // c.shape[0])
        out.append(sv.energy_batch(np.ascontiguousarray(np.tile(c, (reps, 1)))[: max(257, c.shape[0])])[: c.shape[0]])
    return np.concatenate(out)


def _thetas_with_nan_tail(rng, B, K, scale=1.0, extra=8):
    full = np.full((B + extra, K), np.nan)
    full[:B] = rng.uniform(-scale, scale, (B, K))
    return full


def _check_batch(case, sv, th, e, second=True):
    B = th.shape[0]
    assert np.isfinite(e).all()
    idx = _sample(B)
    ref = case.oracle(th[idx])
    assert np.abs(e[idx] - ref).max() < 1e-11 * case.scale, (idx, e[idx] - ref)
    if second:
        e2 = _second_form(sv, th)
        assert np.abs(e - e2).max() < 1e-12 * case.scale


def _form_for(B):
    if B <= 256:
        return "wg"
    if B <= 1024:
        return "staged1"
    return "plain1" if B < 2048 else "rows2"


@pytest.fixture(scope="module")
def h2o(gpu_lib):
    import bench
    ham, gens, hf = bench.build_workload()
    from openvqe_amd.backend import compile_ucc_program
    n = ham.nbqbits
    rx, rz, rc, rp, K = compile_ucc_program(n, gens)
    hf_index = int(sum(1 << (n - 1 - q) for q, v in enumerate(hf) if v)) if not np.isscalar(hf) else int(hf)
    return Case(n, hf_index, rx, rz, rc, rp, K, ham)


@pytest.mark.parametrize("B", [1, 2, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 16385])
def test_headline_workload_every_batch_edge(h2o, B):
    """H2O/STO-3G UCCSD (bench.build_workload, 441 of 16384 amplitudes): wg / staged-1 / unstaged-1 / rows-2 (the headline kernel
    k_sparse_vqe_rows<2>) at each side of their batch thresholds, odd batches (the SPW = 2 tail), the grid-stride wrap (16385 =
    2 x 8192 + 1) and theta rows past B that are NaN"""
    from openvqe_amd.backend import Statevector
    rng = np.random.default_rng(B)
    full = _thetas_with_nan_tail(rng, B, h2o.K)
    with Statevector(h2o.n) as sv:
        sv.set_hamiltonian(h2o.H)
        h2o.program(sv)
        e = sv.energy_batch(full[:B])
        assert sv.sparse_forms() == {_form_for(B)}
        assert sv.program_info()["support"] == 441
        _check_batch(h2o, sv, full[:B], e)


@pytest.mark.parametrize("B", [1, 257, 1025, 2049, 16385])
def test_device_entry_point_equals_the_host_one_and_writes_nothing_past_B(h2o, B):
    """ovqe_energy_batch_device: energies into en[:B] of a NaN-filled tensor of B + 64, theta rows past B NaN — the tail stays NaN bit
    for bit, and the energies equal those through host buffers bit for bit (same kernel)"""
    import torch
    from openvqe_amd.backend import Statevector
    rng = np.random.default_rng(1000 + B)
    full = _thetas_with_nan_tail(rng, B, h2o.K, extra=64)
    th_dev = torch.from_numpy(full).cuda()
    en = torch.full((B + 64,), float("nan"), dtype=torch.float64, device="cuda")
    tail_bits = en[B:].view(torch.int64).cpu().clone()
    with Statevector(h2o.n) as sv:
        sv.set_hamiltonian(h2o.H)
        h2o.program(sv)
        sv.energy_batch_device(B, th_dev.data_ptr(), en.data_ptr())
        torch.cuda.synchronize()
        assert sv.sparse_forms() == {_form_for(B)}
        e_host = sv.energy_batch(full[:B])
    assert torch.equal(en[B:].view(torch.int64).cpu(), tail_bits)
    e_dev = en[:B].cpu().numpy()
    assert np.array_equal(e_dev.view(np.int64), e_host.view(np.int64))
    idx = _sample(B)
    assert np.abs(e_dev[idx] - h2o.oracle(full[idx])).max() < 1e-11 * h2o.scale


@pytest.mark.parametrize("opts, B, form", [({"sparse_rows": 0}, 2049, "plain2"), ({"sparse_spw": 4}, 2051, "plain4"),
                                           ({"sparse_spw": 1}, 8193, "plain1")])
def test_testing_forms_on_the_headline_workload(testing_lib, h2o, opts, B, form):
    """k_sparse_vqe<2> without row tables, <4> (four evaluations per wave, B = 4 x 512 + 3: the tail) and <1> with a grid that
    wraps (8193 work items)"""
    from openvqe_amd.backend import Statevector
    rng = np.random.default_rng(B)
    full = _thetas_with_nan_tail(rng, B, h2o.K)
    with Statevector(h2o.n) as sv:
        for k, v in opts.items():
            sv.set_option(k, v)
        sv.set_hamiltonian(h2o.H)
        h2o.program(sv)
        e = sv.energy_batch(full[:B])
        assert sv.sparse_forms() == {form}
        _check_batch(h2o, sv, full[:B], e)


# ---- support edges --------------------------------------------------------------------------------------------------------------
def _geometry(m):
    """(case, designed support size) of a program whose reachable support has exactly m basis states (m > 4096: 4224)"""
    if m == 1:   # one excitation between two empty orbitals: no op has a pair on the support (no active op at all)
        n, hf, gens, K = 4, 0b0011, [pattern_excitation([2], [3]) + (0,)], 1
    elif m == 2:
        n, hf, gens, K = cascade_geometry(1, 0, 0)
    elif m == 32:
        n, hf, gens, K = cascade_geometry(5, 0, 0)
    elif m == 33:   # 32 + the one state of the block whose bits 0..5 are all set, moved to bit 6
        n, hf, gens, K = cascade_geometry(5, 0, 0)
        gens = gens + [pattern_excitation([0, 1, 2, 3, 4, 5], [6]) + (K,)]
        n, K = 7, K + 1
    elif m == 4064:   # (2^7 - 1) x 2^5: the largest renumbered support
        n, hf, gens, K = cascade_geometry(6, 6, 5)
    elif m == 4095:   # 2^12 - 1: not renumbered, odd
        n, hf, gens, K = cascade_geometry(11, 11, 0)
    elif m == 4096:   # slot 4095 in the 12-bit fields
        n, hf, gens, K = cascade_geometry(12, 0, 0)
    else:   # 4096 + 2^(12-5): beyond the 12-bit slots
        n, hf, gens, K = cascade_geometry(12, 0, 0)
        gens = gens + [pattern_excitation([0, 1, 2, 3, 4, 5], [13]) + (K,)]
        n, K = 14, K + 1
    case = _designed(n, hf, gens, K, seed=m)
    assert len(support_closure(case.hf, case.rx, case.rz, case.rc, case.rp)) == m
    return case


def _two_per_wave_fit(m, case):
    """run_sparse: 2 x (support slots + one cos/sin pair per table entry) within 64 KiB; one table entry per op here (every
    generator of these programs has one active pattern), slots: the support, in rows of 32 when it is renumbered (32 < m <= 4064)"""
    ntab = 1 + int(np.count_nonzero(case.rx[1:] != case.rx[:-1]))
    mp = 32 * -(-m // 32) if 32 < m <= 4064 else m
    return 2 * (((mp + 1) & ~1) * 8 + ntab * 16) <= 64 * 1024


@pytest.mark.parametrize("m", [1, 2, 32, 33, 4064, 4095, 4096])
def test_support_edges_every_energy_form_and_the_gradient(gpu_lib, m):
    from openvqe_amd.backend import Statevector
    case = _geometry(m)
    rng = np.random.default_rng(m)
    with Statevector(case.n) as sv:
        sv.set_hamiltonian(case.H)
        case.program(sv)
        for B in (1, 300, 1100, 2049):
            full = _thetas_with_nan_tail(rng, B, case.K, scale=2.0)
            before = sv.sparse_forms()
            e = sv.energy_batch(full[:B])
            if m == 1:   # no active op: no row tables
                want = {1: "staged1", 300: "staged1", 1100: "plain1", 2049: "plain2"}[B]
            elif B == 2049 and not _two_per_wave_fit(m, case):   # two states per wave would take more than 64 KiB of LDS
                want = "plain1"
            else:
                want = _form_for(B)
            assert sv.sparse_forms() == before | {want}, (B, sv.sparse_forms())
            assert sv.program_info()["support"] == m
            _check_batch(case, sv, full[:B], e, second=B > 256 and B < 2048 or m == 1)
        th = rng.uniform(-2, 2, case.K)
        e, g = sv.energy_gradient(th)
        assert {"grad_staged" if m == 1 else "grad_wg"} <= sv.sparse_forms()
        assert "declined" not in sv.sparse_forms()
    e_ref, g_ref = case.oracle_gradient(th)
    assert abs(e - e_ref) < 1e-11 * case.scale
    assert np.abs(g - g_ref).max() < 1e-11 * case.scale
    if m == 1:
        assert np.all(g == 0.0)


def test_support_beyond_4096_declines_to_the_other_paths(gpu_lib):
    from openvqe_amd.backend import Statevector
    case = _geometry(4224)
    rng = np.random.default_rng(4224)
    th = rng.uniform(-1, 1, (3, case.K))
    with Statevector(case.n) as sv:
        sv.set_hamiltonian(case.H)
        case.program(sv)
        e = sv.energy_batch(th)
        e1 = sv.energy(th[0])
        eg, g = sv.energy_gradient(th[0])
        assert sv.sparse_forms() == {"declined"}
        assert sv.program_info()["support"] == 0
    ref = case.oracle(th)
    assert np.abs(e - ref).max() < 1e-11 * case.scale and abs(e1 - ref[0]) < 1e-11 * case.scale
    e_ref, g_ref = case.oracle_gradient(th[0])
    assert abs(eg - e_ref) < 1e-11 * case.scale and np.abs(g - g_ref).max() < 1e-11 * case.scale


# ---- angle table ----------------------------------------------------------------------------------------------------------------
def _angle_case():
    """shared primitives: one parameter on generators of coefficients +c and -c (one cos/sin entry, the sign in the word), a
    magnitude one ulp larger (its own entry), one parameter on several generators, a parameter whose only op has no pair on the
    support (derivative exactly 0), and JW parity chains"""
    c = 0.7
    c1 = float(np.nextafter(c, 1.0))
    xs6, zs6, cs6 = pattern_excitation([0], [6], chain=[3])
    gens = [([1 << 1], [1 << 1], [c], 0),
            ([1 << 2], [1 << 2], [-c], 0),      # shares the entry of the first, sign in the word
            ([1 << 3], [1 << 3], [c], 0),
            ([1 << 4], [1 << 4], [c1], 0),      # one ulp more: an entry of its own
            pattern_excitation([0], [5], chain=[1, 2]) + (1,),
            ([1 << 1], [1 << 1], [2.5], 2),
            (xs6, zs6, [-v for v in cs6], 1),   # parameter 1 again, opposite signs
            pattern_excitation([8], [9]) + (3,),   # bits 8 and 9 stay clear on the support: no pair
            pattern_excitation([0, 2], [5, 7], chain=[4]) + (2,),
            y_rotation(2) + (4,)]
    return _designed(10, 0b1, gens, 5, seed=77)


@pytest.mark.parametrize("kind", ["random", "large", "quarter_turns"])
def test_angle_table_sharing_and_extreme_angles(gpu_lib, kind):
    from openvqe_amd.backend import Statevector
    case = _angle_case()
    rng = np.random.default_rng(len(kind))
    B = 2049
    if kind == "random":
        th = rng.uniform(-3, 3, (B, case.K))
    elif kind == "large":
        th = rng.uniform(-1e3, 1e3, (B, case.K))
        th[:, 0] = 1e3 * np.sign(th[:, 0])
    else:
        th = rng.integers(-8, 9, (B, case.K)) * (np.pi / 2)
    with Statevector(case.n) as sv:
        sv.set_hamiltonian(case.H)
        case.program(sv)
        e_rows = sv.energy_batch(th)
        assert sv.sparse_forms() == {"rows2"}
        idx = _sample(B)
        assert np.abs(e_rows[idx] - case.oracle(th[idx])).max() < 1e-11 * case.scale
        e_wg = np.concatenate([sv.energy_batch(th[c0:c0 + 256]) for c0 in range(0, B, 256)])
        e_st = sv.energy_batch(np.ascontiguousarray(th[:1000]))
        assert sv.sparse_forms() == {"rows2", "wg", "staged1"}
        assert np.abs(e_rows - e_wg).max() < 1e-12 * case.scale
        assert np.abs(e_rows[:1000] - e_st).max() < 1e-12 * case.scale
        for b in (0, B // 2, B - 1):
            eg, g = sv.energy_gradient(th[b])
            e_ref, g_ref = case.oracle_gradient(th[b])
            assert abs(eg - e_ref) < 1e-11 * case.scale
            assert np.abs(g - g_ref).max() < 1e-11 * case.scale, (g, g_ref)
            assert g[3] == 0.0
        assert "grad_wg" in sv.sparse_forms()


# ---- gradient forms -------------------------------------------------------------------------------------------------------------
def _many_pairs_case():
    """m = 4096 (Y on twelve bits) and the twelve Y rotations again on new parameters: 24 ops of 2048 pairs each — the staged
    one-wave gradient form would need 2 x 32 KiB + ~196 KiB of LDS"""
    n, hf, gens, K = cascade_geometry(12, 0, 0)
    gens = gens + [y_rotation(b) + (K + b - 1,) for b in range(1, 13)]
    return _designed(n, hf, gens, K + 12, seed=4096)


@pytest.mark.parametrize("geometry, form", [("angles", "grad_staged"), ("many_pairs", "grad_plain")])
def test_one_wave_gradient_forms(testing_lib, geometry, form):
    """k_sparse_grad<true> / <false> (the workgroup form switched off: testing option "sparse_wg") against the oracle gradient and
    against the workgroup form"""
    from openvqe_amd.backend import Statevector
    case = _angle_case() if geometry == "angles" else _many_pairs_case()
    rng = np.random.default_rng(7)
    th = rng.uniform(-2, 2, case.K)
    with Statevector(case.n) as sv:
        sv.set_hamiltonian(case.H)
        case.program(sv)
        e_wg, g_wg = sv.energy_gradient(th)
        assert sv.sparse_forms() == {"grad_wg"}
        sv.set_option("sparse_wg", 0)
        e, g = sv.energy_gradient(th)
        assert sv.sparse_forms() == {"grad_wg", form}
    e_ref, g_ref = case.oracle_gradient(th)
    assert abs(e - e_ref) < 1e-11 * case.scale and np.abs(g - g_ref).max() < 1e-11 * case.scale
    assert abs(e - e_wg) < 1e-12 * case.scale and np.abs(g - g_wg).max() < 1e-12 * case.scale


# ---- angle tables at the LDS budget -----------------------------------------------------------------------------------------------
def _deep_case(ntab, distinct):
    """m = 32 (Y on bits 1..5) and inactive excitations between the empty bits 6, 7, 8 (alternating x masks, one table entry each) up
    to ntab table entries: 32 x 8 + ntab x 16 bytes of LDS per evaluation (150 KiB = 153600: ntab = 9584 fits, 9585 does not).
    distinct: every padding entry its own magnitude (>= 4095 distinct angles: no row tables, no workgroup form)"""
    n, hf, gens, K = cascade_geometry(5, 0, 0)
    npad = ntab - len(gens)
    for j in range(npad):
        occ, virt = ([6], [7]) if j % 2 == 0 else ([7], [8])
        xs, zs, cs = pattern_excitation(occ, virt)
        if distinct:
            cs = [v * (1.0 + j * 2.0 ** -30) for v in cs]
        gens.append((xs, zs, cs, K + j % 11))
    case = _designed(9, hf, gens, K + 11, seed=ntab)
    return case


@pytest.mark.parametrize("ntab, distinct", [(9584, False), (9585, True)])
def test_angle_table_at_the_lds_budget(gpu_lib, ntab, distinct):
    """per-evaluation LDS just inside / just past 150 KiB: every batch size is served (a compact form, or the other paths when no
    compact form fits: no error) and matches the oracle, and so does the gradient"""
    from openvqe_amd.backend import Statevector
    case = _deep_case(ntab, distinct)
    rng = np.random.default_rng(ntab)
    with Statevector(case.n) as sv:
        sv.set_hamiltonian(case.H)
        case.program(sv)
        for B in (1, 256, 257, 1025, 2048):
            th = rng.uniform(-2, 2, (B, case.K))
            e = sv.energy_batch(th) if B > 1 else np.array([sv.energy(th[0])])
            forms = sv.sparse_forms()
            if distinct:
                assert forms == {"declined"}
            else:
                assert (_form_for(B) if B <= 256 else "plain1") in forms and "declined" not in forms
            idx = np.array(sorted({0, B // 2, B - 1}))
            assert np.abs(e[idx] - case.oracle(th[idx])).max() < 1e-11 * case.scale
        th = rng.uniform(-2, 2, case.K)
        eg, g = sv.energy_gradient(th)
    e_ref, g_ref = case.oracle_gradient(th)
    assert abs(eg - e_ref) < 1e-11 * case.scale and np.abs(g - g_ref).max() < 1e-11 * case.scale
