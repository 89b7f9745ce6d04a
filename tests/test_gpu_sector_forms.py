"""Every kernel form of the sector path (openvqe_amd/csrc/sv_sector.hpp, selection in sector_host.inc) at 14 - 20 qubits: every test
sets the options that force a form, evaluates at least three parameter vectors (the last one zero), asserts through
``sector_forms()`` / ``sector_choices()`` / ``program_info()`` that the form ran, and holds the result against the C oracle
(energies, 1e-10 max(1, |H|_1)) and the exact support-only adjoint pass of tests/sector_cases.py (every gradient component,
1e-10 max(1, |H|_1)).  Forms that share their tables are held against each other as the existing tests establish: energies bit for
bit (second against third sweep form, 24-bit against 32-bit <H> words), gradients to 1e-12 max(1, |H|_1) (their sums are reordered).
A fresh handle per configuration: the form word of a handle accumulates until the next program is set.

REACHABLE ONLY AT FULL SIZE (tests/test_gpu_fullsize.py keeps them): the first sweep form without staging ahead at more than 64
threads needs one op with more than 4096 pairs in one tile, i.e. a tile above 8192 amplitudes on which one op touches every
amplitude — the 20-qubit case below has such tiles (8820 amplitudes) but its widest op, a single excitation, touches half of a
tile's amplitudes at most (two of the four settings of its two bits), 2205 pairs; here the variant is reached with 64 threads, where
it is the only one.  Grids beyond 65535 tiles need 22 qubits and more."""
import numpy as np
import pytest

from tests import sector_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture
def testing_lib(gpu_lib, monkeypatch):
    """the OVQE_TESTING build of the same source: it also takes the options that pick a kernel form"""
    from openvqe_amd import _lib
    monkeypatch.setattr(_lib, "LIB_PATH", _lib.TESTING_LIB_PATH)
    monkeypatch.setattr(_lib, "_lib", None)
    return _lib.lib()


INFO = ("sector_support", "sector_sweeps", "sector_h_sweeps", "sector_tile_bits", "sector_h_tile_bits", "sector_pair_slot_bits",
        "sector_max_tile", "sector_h_max_tile", "sector_h_max_dict", "sector_h_dict_entries", "sector_ordered_sweeps")


def _open(case, opts):
    from openvqe_amd.backend import Statevector
    sv = Statevector(case.n)
    for k, v in {"force_path": 2, "sector_min_qubits": 8, **opts}.items():
        sv.set_option(k, v)
    sv.set_hamiltonian(case.ham)
    sv.set_ucc_program(case.gens, case.hf)
    return sv


def _report(what, case, sv, dev):
    info = sv.program_info()
    print(f"{what} | {case.name} | forms {sorted(sv.sector_forms())} | choices {sorted(sv.sector_choices())} | "
          + " ".join(f"{k[7:]}={info[k]}" for k in INFO) + f" | largest deviation / bound {dev:.3e}")
    return info


def energies(case, opts, thetas, what):
    """energies of a fresh handle at ``thetas`` (twice: the tables are built at the second evaluation) against the C oracle
    -> (energies from the tables, forms, choices, info)"""
    with _open(case, opts) as sv:
        for t in thetas[:2]:
            sv.energy(t)
        got = [sv.energy(t) for t in thetas]
        dev = max(abs(e - case.energy(t)) for e, t in zip(got, thetas)) / (1e-10 * case.bound)
        info = _report(what, case, sv, dev)
        forms, choices = sv.sector_forms(), sv.sector_choices()
    assert info["sector_support"] == len(case.support), info
    assert dev < 1.0, (what, dev)
    return got, forms, choices, info


def batches(case, opts, thetas, what, sizes=(8, 3)):
    """``energy_batch`` of a fresh handle against the C oracle -> (forms, choices).  The first batch has four states or more, which builds
    the tables at once: a batch of three on a fresh handle would be served one state at a time and build them on the way."""
    pool = np.stack([thetas[k % len(thetas)] * (1.0 - 0.1 * (k // len(thetas))) for k in range(max(sizes))])
    want = np.array([case.energy(t) for t in pool])
    with _open(case, opts) as sv:
        dev = 0.0
        for B in sizes:
            for _ in range(2):
                got = sv.energy_batch(pool[:B])
            dev = max(dev, np.abs(got - want[:B]).max() / (1e-10 * case.bound))
        _report(what + f" batches {sizes}", case, sv, dev)
        forms, choices = sv.sector_forms(), sv.sector_choices()
    assert dev < 1.0, (what, dev)
    return forms, choices


def gradients(case, opts, thetas, what):
    """``energy_gradient`` of a fresh handle against the oracle's energy and every component of the reference
    -> (list of (energy, grad), forms, choices, info)"""
    with _open(case, opts) as sv:
        got = [sv.energy_gradient(t) for t in thetas]
        dev = 0.0
        for (e, g), t in zip(got, thetas):
            e_ref, g_ref = case.gradient(t)
            dev = max(dev, abs(e - case.energy(t)) / (1e-10 * case.bound), np.abs(g - g_ref).max() / (1e-10 * case.bound))
        info = _report(what + " gradient", case, sv, dev)
        forms, choices = sv.sector_forms(), sv.sector_choices()
    assert info["sector_support"] == len(case.support), info
    assert dev < 1.0, (what, dev)
    return got, forms, choices, info


def _sizes(choices, group):
    return {int(c.split("_")[1]) for c in choices if c.startswith(group + "_") and c.split("_")[1].isdigit()}


# ---- 1. sweep form x workgroup size --------------------------------------------------------------------------------------------------
SWEEP_CONFIGS = [(1, 64), (1, 256), (1, 512), (1, 1024), (2, 256), (2, 512), (2, 1024), (3, 0), (3, 1024), (4, 0), (4, 1024)]


def _forward_expectation(sweep, threads):
    if sweep == 1:      # k_sector_sweep<NT>; two chunks of pair words ahead above 64 threads (no op of these tiles has 4096 pairs)
        return {"sweep_pairs"}, {"sweep_pairs_ahead" if threads > 64 else "sweep_pairs_plain", f"sweep_{threads}"}
    if sweep == 2:      # k_sector_sweep2<NT>, scatter indices in LDS (fewer than 768 tiles)
        return {"sweep_wide"}, {"scatter_in_lds", f"sweep_{threads}"}
    return {"sweep_streams"}, {"scatter_in_lds", "sweep_1024"}     # k_sector_sweep3<1024>: automatic size below 768 tiles = 1024


STREAM_WAVES = 2      # "sector_stream_waves": tiles of a few dozen amplitudes get no streams by themselves (fewer than 24 pairs per op)


@pytest.mark.parametrize("sweep,threads", SWEEP_CONFIGS)
@pytest.mark.parametrize("m,o,bits", [(7, 3, 8), (7, 3, 10), (8, 3, 8), (8, 3, 10)])
def test_sweep_form_and_workgroup_size(testing_lib, m, o, bits, sweep, threads):
    """(7,3) and (8,3) with tiles of 8 and 10 index bits: several sweeps, tile populations that are no multiple of 64 and some
    below a wave.  Forwards: the form and size asked for; the streams of the third form are forced on these small tiles with two
    waves, and a sweep whose runs would hold fewer than two ops on average keeps the second form (build_wave_streams), so there the
    second form may appear next to the third, never the first.  Batches of 3 and 8: without the 64-bit words ("sector_sweep" 1) one
    evaluation at a time on the first form, else k_sector_sweep2<512> with late scatter indices WHATEVER "sector_sweep" says — the
    batch's workgroups are 512 threads and the streams are planned for 1024 (so "sector_sweep" 4 adds nothing to a batch).
    Backwards: "sector_adjoint" 1 -> k_sector_adjoint<NT>, NT the largest of 1024 / 512 / 256 not above max(threads, 256) whose
    per-wave partial sums fit LDS; 2 -> k_sector_adjoint2<1024>; 3 -> k_sector_adjoint3<1024> where the streams exist
    ("sector_sweep" >= 3), else as 2; without the 64-bit words always the first."""
    case = sc.molecule(m, o)
    thetas = case.thetas(3)
    opts = {"sector_bits": bits, "sector_sweep": sweep, "sector_threads": threads}
    if sweep >= 3:
        opts["sector_stream_waves"] = STREAM_WAVES
    what = f"sweep {sweep} threads {threads} bits {bits}"
    forms_want, choices_want = _forward_expectation(sweep, threads)
    _, forms, choices, info = energies(case, opts, thetas, what)
    assert info["sector_tile_bits"] == bits and info["sector_sweeps"] > 1 and info["sector_pair_slot_bits"] == 15, info
    ran = forms & {"sweep_pairs", "sweep_wide", "sweep_streams", "sweep_regular"}
    assert forms_want <= ran <= forms_want | ({"sweep_wide"} if sweep >= 3 else set()), forms
    assert {c for c in choices if c.startswith(("sweep_", "scatter_"))} == choices_want, choices
    assert "pair_builder_dense_map" in choices and "pair_builder_search" not in choices
    forms, choices = batches(case, opts, thetas, what)
    if sweep == 1:
        assert forms & {"sweep_pairs", "sweep_wide", "sweep_streams"} == {"sweep_pairs"} and _sizes(choices, "sweep") == {threads}
    else:
        assert forms & {"sweep_pairs", "sweep_wide", "sweep_streams"} == {"sweep_wide"}, forms
        assert _sizes(choices, "sweep") == {512} and "scatter_late" in choices and "scatter_in_lds" not in choices, choices
    by_adjoint = {}
    for adjoint in (1, 2, 3):
        got, forms, choices, _ = gradients(case, dict(opts, sector_adjoint=adjoint), thetas, what + f" adjoint {adjoint}")
        back = forms & {"adjoint_pairs", "adjoint_wide", "adjoint_streams", "adjoint_regular"}
        if adjoint == 1 or sweep == 1:
            assert back == {"adjoint_pairs"}, (adjoint, forms)
            size = _sizes(choices, "adjoint")
            assert len(size) == 1 and size <= {s for s in (256, 512, 1024) if s <= max(threads, 256)}, (adjoint, choices)
        else:
            if adjoint == 3 and sweep >= 3:
                assert {"adjoint_streams"} <= back <= {"adjoint_streams", "adjoint_wide"}, (adjoint, forms)
            else:
                assert back == {"adjoint_wide"}, (adjoint, forms)
            assert _sizes(choices, "adjoint") == {1024}, choices
        assert {"apply_atomic", "apply_512"} <= choices and not {"apply_sequential", "apply_1024"} & choices, choices
        by_adjoint[adjoint] = got
    for adjoint in (2, 3):      # the same lambda, the partial sums added in another order
        for (e1, g1), (e2, g2) in zip(by_adjoint[1], by_adjoint[adjoint]):
            assert abs(e1 - e2) < 1e-12 * case.bound and np.abs(g1 - g2).max() < 1e-12 * case.bound, adjoint


@pytest.mark.parametrize("m,o,bits", [(7, 3, 8), (8, 3, 10)])
def test_sweep_forms_on_the_same_tables_agree(testing_lib, m, o, bits):
    """tables built under "sector_sweep" 3 serve all three forms: third == second bit for bit (a pair is rotated by the same
    arithmetic, every slot sees its ops in program order), the first within 1e-13 max(1, |H|_1) of them"""
    case = sc.molecule(m, o)
    thetas = case.thetas(3)
    got = {}
    with _open(case, {"sector_bits": bits, "sector_sweep": 3, "sector_stream_waves": STREAM_WAVES}) as sv:
        for t in thetas[:2]:
            sv.energy(t)
        for sweep in (3, 2, 1):
            sv.set_option("sector_sweep", sweep)
            got[sweep] = [sv.energy(t) for t in thetas]
        forms = sv.sector_forms()
        _report("same tables", case, sv, max(abs(e - case.energy(t)) for e, t in zip(got[3], thetas)) / (1e-10 * case.bound))
    assert {"sweep_pairs", "sweep_wide", "sweep_streams"} <= forms, forms
    assert got[3] == got[2]
    assert max(abs(a - b) for a, b in zip(got[1], got[2])) < 1e-13 * case.bound
    assert max(abs(e - case.energy(t)) for e, t in zip(got[1], thetas)) < 1e-10 * case.bound


# ---- 2. many tiles -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threads", [0, 1024])
def test_many_tiles_take_512_threads_late_scatter_indices_and_the_largest_first_order(gpu_lib, threads):
    """(8,4) with tiles of 6 index bits: 1024 tiles per sweep, most of them empty or tiny.  From 768 tiles on the automatic selection
    takes k_sector_sweep2<512> with the scatter indices read late; every sweep has 512 tiles or more, so all of them walk their tiles
    largest first.  "sector_threads" 1024 holds the indices in LDS (k_sector_sweep2<1024>: tiles this small get no streams)."""
    case = sc.molecule(8, 4)
    thetas = case.thetas(3)
    what = f"many tiles threads {threads}"
    _, forms, choices, info = energies(case, {"sector_bits": 6, "sector_threads": threads}, thetas, what)
    assert info["sector_tile_bits"] == 6 and info["sector_ordered_sweeps"] == info["sector_sweeps"] > 1, info
    if threads == 0:
        assert forms & {"sweep_pairs", "sweep_wide", "sweep_streams"} == {"sweep_wide"}, forms
        assert {c for c in choices if c.startswith(("sweep_", "scatter_"))} == {"scatter_late", "sweep_512"}, choices
    else:
        assert forms & {"sweep_pairs", "sweep_wide", "sweep_streams"} == {"sweep_wide"}, forms
        assert {c for c in choices if c.startswith(("sweep_", "scatter_"))} == {"scatter_in_lds", "sweep_1024"}, choices
    gradients(case, {"sector_bits": 6, "sector_threads": threads}, thetas, what)


# ---- 3. lambda = H psi -------------------------------------------------------------------------------------------------------------
def _ground_state(case, opts, what):
    """sector_ground_state on a fresh handle -> energy; the vector it leaves is an eigenvector of the Hamiltonian restricted to the
    support (residual by sector_cases.apply_on_support below 1e-6, the solver's own bar) and lies on the support"""
    with _open(case, opts) as sv:
        e, res, _ = sv.sector_ground_state(tol=1e-12)
        vec = sv.get_state()
        choices = sv.sector_choices()
    idx = case.support.astype(np.int64)
    on = vec[idx]
    assert abs(np.linalg.norm(on) - 1.0) < 1e-12 and abs(np.linalg.norm(vec) - 1.0) < 1e-12
    r = sc.apply_on_support(case.support, on.astype(np.complex128), case.hx, case.hz, case.hc) + (case.ham.constant_coeff - e) * on
    print(f"{what} | {case.name} | ground state {e:.12f} residual {np.linalg.norm(r):.2e} (solver: {res:.2e}) | choices {sorted(choices)}")
    assert np.linalg.norm(r) < 1e-6 and res < 1e-6
    return e, choices


@pytest.mark.parametrize("m,o,h_bits,mode,size", [(8, 4, 4, "apply_sequential", "apply_512"), (8, 4, 0, "apply_atomic", "apply_512"),
                                                  (9, 4, 17, "apply_atomic", "apply_1024")])
def test_lambda_store_modes_and_workgroup_sizes(gpu_lib, m, o, h_bits, mode, size):
    """k_sector_apply.  (8,4), K = 4900: <H> tiles of 4 index bits hold at most 6 members of the sector, K >= 512 * 6, so the sweeps
    run in sequence with plain stores (modes 2 then 1), several of them; automatic tiles (8 bits, up to 36 members) take the LDS
    atomics behind a memset.  (9,4) with "sector_h_bits" 17: two tiles of 7938 exceed the 7600 of SEC_HTILE_LDS_CAP, the tile bits
    come back as 16 or fewer, and tiles of about 4000 need more than 48 KiB for lambda's second tile: 1024 threads.
    The ground state's energy is below every ansatz energy and equal in every mode of the same Hamiltonian."""
    case = sc.molecule(m, o)
    thetas = case.thetas(3)
    opts = {"sector_h_bits": h_bits}
    what = f"lambda h_bits {h_bits}"
    _, _, _, info = energies(case, opts, thetas, what)
    got, _, choices, info = gradients(case, opts, thetas, what)
    assert {mode, size} == {c for c in choices if c.startswith("apply_")}, choices
    if h_bits == 4:
        assert info["sector_h_tile_bits"] == 4 and info["sector_h_sweeps"] > 1 and info["sector_support"] >= 512 * info["sector_h_max_tile"], info
    elif h_bits == 17:
        assert info["sector_h_tile_bits"] <= 16 and 3000 < info["sector_h_max_tile"] <= 7600, info
    else:
        assert info["sector_h_tile_bits"] == info["sector_tile_bits"] and info["sector_support"] < 512 * info["sector_h_max_tile"], info
    e0, choices = _ground_state(case, opts, what)
    assert {mode, size} == {c for c in choices if c.startswith("apply_")}, choices
    assert all(e0 <= e + 1e-12 for e, _ in got)
    if (m, o) == (8, 4):
        _GROUND.setdefault("e", e0)
        assert abs(e0 - _GROUND["e"]) < 1e-9


_GROUND = {}


# ---- 4. coding of the materialised <H> at the dictionary's boundaries ----------------------------------------------------------------
CODING = [(1023, {}, "h_packed24"), (1024, {}, "h_dict32"), (4096, {}, "h_dict32"), (4097, {}, "h_explicit_overflow"),
          (4097, {"sector_dict": 3}, "h_explicit_sample_failed"), (4097, {"sector_dict": 0}, "h_explicit_no_dict"),
          (1023, {"sector_dict": 0}, "h_explicit_no_dict")]


@pytest.mark.parametrize("entries,extra,outcome", CODING, ids=[f"{e}-{o}" for e, _, o in CODING])
def test_hamiltonian_coding_at_the_dictionary_boundaries(gpu_lib, entries, extra, outcome):
    """the counted-magnitude Hamiltonian (tests/sector_cases.py) with "sector_h_bits" 13: ONE <H> sweep whose dictionary has exactly
    ``entries`` magnitudes.  1023: 24-bit packed words (the null element is entry 1023, the last a 10-bit field names); 1024: 32-bit
    words; 4096: still a dictionary (SEC_DICT_MAX, the null element one past the LDS block's last magnitude); 4097: explicit values;
    with a sample of every 4096th value the sample fits and the stream does not (k_sec_words_slots); "sector_dict" 0: no dictionary."""
    case = sc.counted_case(sc.COUNTED_GROUPS[entries])
    thetas = case.thetas(3, scale=0.6)
    opts = dict({"sector_h_bits": 13}, **extra)
    what = f"coding {entries} {outcome}"
    got, _, choices, info = energies(case, opts, thetas, what)
    assert info["sector_h_sweeps"] == 1 and info["sector_h_tile_bits"] == 13 and info["sector_h_max_tile"] == sc.COUNTED_SUPPORT, info
    assert info["sector_pair_slot_bits"] == 15, info
    assert {c for c in choices if c.startswith("h_")} == {outcome}, choices
    coded = outcome in ("h_packed24", "h_dict32")
    assert info["sector_h_max_dict"] == info["sector_h_dict_entries"] == (entries if coded else 0), info
    for e, t in zip(got, thetas):        # <psi|H|psi> on the oracle's state by the support-only product
        _, psi = case.oracle(t)
        on = psi[case.support.astype(np.int64)]
        want = float(np.vdot(on, sc.apply_on_support(case.support, on, case.hx, case.hz, case.hc)).real) + case.ham.constant_coeff
        assert abs(e - want) < 1e-10 * case.bound
    gradients(case, opts, thetas, what)
    batches(case, opts, thetas, what, sizes=(4, 3))


def test_packed_words_equal_the_32_bit_words_at_1023_entries(testing_lib):
    """1023 entries with "sector_h_pack" 0 keeps the 32-bit words: energies and batches equal the packed ones bit for bit"""
    case = sc.counted_case(sc.COUNTED_GROUPS[1023])
    thetas = case.thetas(3, scale=0.6)
    out = {}
    for pack, outcome in ((1, "h_packed24"), (0, "h_dict32")):
        opts = {"sector_h_bits": 13, "sector_h_pack": pack}
        got, _, choices, _ = energies(case, opts, thetas, f"pack {pack}")
        assert {c for c in choices if c.startswith("h_")} == {outcome}, choices
        with _open(case, opts) as sv:
            out[pack] = (got, sv.energy_batch(np.stack(thetas)))
    assert out[1][0] == out[0][0] and np.array_equal(out[1][1], out[0][1])


# ---- 5. slot bits and tile caps ----------------------------------------------------------------------------------------------------
def test_slot_bits_follow_the_widest_op(gpu_lib):
    """the pattern field of a pair word takes what the widest op needs: 15 slot bits up to two patterns — single-string rotations, and
    the JW excitations of UCCSD, whose 2 or 8 strings fuse into tables of two patterns —, 14 up to eight (the reference's QUCCSD
    templates on pair words, "sector_regular" 0), 13 beyond (one generator whose angle differs on all 16 settings of four bits)"""
    case = sc.molecule(7, 3)
    assert energies(case, {}, case.thetas(3), "slot bits uccsd")[3]["sector_pair_slot_bits"] == 15
    case = sc.counted_case(150)
    _, forms, _, info = energies(case, {"sector_h_bits": 13}, case.thetas(3, scale=0.6), "slot bits single strings")
    assert info["sector_pair_slot_bits"] == 15 and forms & {"sweep_wide", "sweep_streams"}, (info, forms)
    case = sc.many_pattern_case()
    thetas = case.thetas(3, scale=0.6)
    assert energies(case, {}, thetas, "slot bits sixteen patterns")[3]["sector_pair_slot_bits"] == 13
    gradients(case, {}, thetas, "slot bits sixteen patterns")
    q = _quccsd()
    with _open_gates(q, {"sector_regular": 0}) as sv:
        got = [sv.energy(t) for t in q["thetas"]]
        got = [sv.energy(t) for t in q["thetas"]]
        info, forms = sv.program_info(), sv.sector_forms()
    assert info["sector_pair_slot_bits"] == 14 and info["sector_regular_slot_bits"] == 0 and "sweep_regular" not in forms, (info, forms)
    assert max(abs(e - w) for e, w in zip(got, q["want"])) < 1e-10 * q["bound"]


def test_tile_cap_lowers_the_tile_bits(gpu_lib):
    """(8,4) from tiles of 12 index bits (the cap has a floor of 64 amplitudes, the automatic 8-bit tiles hold 40): with the largest
    tile T at the default cap, "sector_tile_cap" = T keeps the tile bits and T - 1 lowers them (the loop that otherwise runs only at
    20 qubits with "sector_bits" 18)"""
    case = sc.molecule(8, 4)
    thetas = case.thetas(3)
    _, _, _, base = energies(case, {"sector_bits": 12}, thetas, "tile cap default")
    T, M = base["sector_max_tile"], base["sector_tile_bits"]
    assert T > 64 and M == 12, base
    _, _, _, same = energies(case, {"sector_bits": 12, "sector_tile_cap": T}, thetas, f"tile cap {T}")
    _, _, _, lower = energies(case, {"sector_bits": 12, "sector_tile_cap": T - 1}, thetas, f"tile cap {T - 1}")
    assert (same["sector_tile_bits"], same["sector_max_tile"]) == (M, T), same
    assert lower["sector_tile_bits"] < M and lower["sector_max_tile"] < T, lower
    gradients(case, {"sector_bits": 12, "sector_tile_cap": T - 1}, thetas, f"tile cap {T - 1}")


def test_tiles_above_8192_amplitudes_use_slot_bit_13(gpu_lib):
    """(10,5) with the single excitations alone, "sector_bits" 17, "sector_tile_cap" 14000: three index bits outside a tile leave
    populations of 5292, 7056 or 8820 — above 8192, so slot indices need bit 13, which two-string ops provide (15 slot bits) —
    and tiles of 17 bits are built by the binary-search builder.  Two tiles of that size do not fit the backward sweeps' LDS:
    energy_gradient leaves the tables (no backward form is reported) and still matches the reference."""
    case = sc.molecule(10, 5, singles_only=True, one_body=True)
    thetas = case.thetas(3)
    opts = {"sector_bits": 17, "sector_tile_cap": 14000}
    _, forms, choices, info = energies(case, opts, thetas, "large tiles")
    assert info["sector_tile_bits"] == 17 and info["sector_pair_slot_bits"] >= 14 and 8192 < info["sector_max_tile"] <= 8820, info
    assert "pair_builder_search" in choices and "pair_builder_dense_map" not in choices, choices
    assert forms & {"sweep_pairs", "sweep_wide", "sweep_streams"}, forms
    _, forms, _, _ = gradients(case, opts, thetas, "large tiles")
    assert not forms & {"adjoint_pairs", "adjoint_wide", "adjoint_streams", "adjoint_regular"}, forms


def _quccsd(m=7, o=3):
    """the reference's QUCCSD gate list on a synthetic molecule with the C oracle's gate-by-gate energies at three parameter vectors"""
    key = ("quccsd", m, o)
    if key not in _GROUND:
        from openvqe_amd import fermion
        from openvqe_amd.backend import GATE_OPCODES
        from openvqe_amd.common_files.circuit import quccsd_gate_list
        from oracle import cref
        n = 2 * m
        ham, _, hf = fermion.synthetic_molecule(m, o, seed=500 + m)
        gates, K, _ = quccsd_gate_list(m, o, 2)
        rng = np.random.default_rng(50 * m + o)
        thetas = [rng.uniform(-0.4, 0.4, K) for _ in range(2)] + [np.zeros(K)]
        hx, hz, hc = ham.packed()
        opc = [GATE_OPCODES[g[0]] for g in gates]
        b0 = [n - 1 - g[1][0] for g in gates]
        b1 = [n - 1 - g[1][1] if len(g[1]) > 1 else 0 for g in gates]
        want = [cref.gate_energy(n, hf, opc, b0, b1, [g[2] for g in gates], [g[3] for g in gates], [g[4] for g in gates], th, hx, hz,
                                 hc.real.copy(), ham.constant_coeff)[0] for th in thetas]
        _GROUND[key] = dict(n=n, ham=ham, hf=hf, gates=gates, K=K, thetas=thetas, want=want, bound=max(1.0, float(np.abs(hc).sum())))
    return _GROUND[key]


def _open_gates(q, opts):
    from openvqe_amd.backend import Statevector
    sv = Statevector(q["n"])
    for k, v in {"force_path": 2, "sector_min_qubits": 8, **opts}.items():
        sv.set_option(k, v)
    sv.set_hamiltonian(q["ham"])
    sv.set_gate_program(q["gates"], q["K"], q["hf"])
    return sv


# ---- 6. regular supports -----------------------------------------------------------------------------------------------------------
REGULAR = [{"sector_reg_threads": 128}, {"sector_reg_threads": 256}, {"sector_reg_threads": 512}, {"sector_reg_threads": 1024},
           {"sector_reg_runs": 0}, {"sector_reg_pairs": 0}, {"sector_reg_adjoint": 0}, {"sector_regular": 3}]


@pytest.mark.parametrize("opts", REGULAR, ids=["-".join(f"{k[7:]}={v}" for k, v in o.items()) for o in REGULAR])
def test_regular_support_sweeps(gpu_lib, opts):
    """the reference's QUCCSD templates at 14 qubits: the support is the spin-parity quarter of the register and the sweeps run from bit
    arithmetic (k_sector_sweep_reg<NT>, NT = "sector_reg_threads"; k_sector_adjoint_reg<256>) — energies against the C oracle's
    gate-by-gate execution (1e-10 max(1, |H|_1)), gradients against the dense-state adjoint pass of the same handle (1e-11), the
    bounds of tests/test_gpu_sector.py::test_sector_on_the_reference_quccsd_templates"""
    q = _quccsd()
    n, thetas, want, bound = q["n"], q["thetas"], q["want"], q["bound"]
    with _open_gates(q, opts) as sv:
        got = [sv.energy(t) for t in thetas]
        got = [sv.energy(t) for t in thetas]
        eg = [sv.energy_gradient(t) for t in thetas]
        forms, choices, info = sv.sector_forms(), sv.sector_choices(), sv.program_info()
        sv.set_option("sector", 0)
        eg_dense = [sv.energy_gradient(t) for t in thetas]
    dev = max(abs(e - w) for e, w in zip(got, want)) / (1e-10 * bound)
    print(f"regular {opts} | forms {sorted(forms)} | choices {sorted(choices)} | slot bits {info['sector_regular_slot_bits']} "
          f"tile bits {info['sector_tile_bits']} | largest deviation / bound {dev:.3e}")
    assert info["sector_support"] == (1 << n) // 4 and info["sector_regular_slot_bits"] > 0, info
    assert "sweep_regular" in forms and not forms & {"sweep_pairs", "sweep_wide", "sweep_streams"}, forms
    threads = opts.get("sector_reg_threads", 256)
    if opts.get("sector_reg_adjoint", 1):
        assert forms & {"adjoint_pairs", "adjoint_wide", "adjoint_streams", "adjoint_regular"} == {"adjoint_regular"}, forms
        assert _sizes(choices, "regular") == {threads, 256}, choices       # (k_sector_adjoint_reg has the one size)
    else:
        assert "adjoint_regular" not in forms and forms & {"adjoint_pairs", "adjoint_wide", "adjoint_streams"}, forms
        assert _sizes(choices, "regular") == {threads}, choices
    assert dev < 1.0
    for (e, g), (ed, gd), w in zip(eg, eg_dense, want):
        assert abs(e - w) < 1e-10 * bound and abs(ed - w) < 1e-10 * bound
        assert np.abs(g - gd).max() < 1e-11 * bound


def test_a_handle_that_never_took_the_sector_path_reports_nothing(gpu_lib):
    """"sector" 0: no form, no choice, and zeros in the sector fields of program_info"""
    case = sc.molecule(7, 2)
    with _open(case, {"sector": 0}) as sv:
        for t in case.thetas(3):
            assert abs(sv.energy(t) - case.energy(t)) < 1e-10 * case.bound
        sv.energy_gradient(case.thetas(3)[0])
        info = sv.program_info()
        assert not sv.sector_forms() and not sv.sector_choices()
    assert all(info[k] == 0 for k in INFO), info
