"""GPU tests of the energy spread S = ||(H - omega) psi||^2 — energy variance and folded-spectrum cost — with energies and exact gradients
of a batch (ovqe_spread_gradient_batch, ovqe_spread_info: k_sparse_spread_batch in csrc/sv_sparse.hpp, spread_host.inc, abi_spread.inc,
sv_spread_host.hpp) and of ``excited.folded_spectrum`` on top of them.

Bounds (tests/spread_cases.py): with N = |w_energy| ||H||_1 + |w_spread| W^2, W = ||H||_1 + |constant| + |omega| (variance mode: |omega| at
||H||_1) and C of tests/gradbatch_cases.py, 1e-10 N max(1, C) against the checker and 1e-12 N max(1, C) against another call on the same
handle.  Every path-1 call is held to ``spread_cases.check_info``: the restated layout and planner."""
import ctypes

import numpy as np
import pytest

from openvqe_amd import excited
from tests import gradbatch_cases as gc
from tests import hessian_cases, metric_cases
from tests import spread_cases as sp

pytestmark = pytest.mark.gpu

WE, WS = 0.3, 1.0     # the mixed weights of the tests


@pytest.fixture(scope="module")
def SV(gpu_lib):
    from openvqe_amd.backend import Statevector
    return Statevector


@pytest.fixture(scope="module")
def h4():
    return sp.molecule("H4")


@pytest.fixture(scope="module")
def lih():
    return sp.molecule("LiH")


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.int64), np.ascontiguousarray(b, np.float64).view(np.int64))


def _call(sv, thetas, omega=None, we=WE, ws=WS):
    """spread_gradient_batch with the checks every result gets -> (costs, grads, energies, spreads, info)"""
    thetas = np.ascontiguousarray(thetas, np.float64)
    c, g, e, s = sv.spread_gradient_batch(thetas, omega, we, ws)
    info = sv.spread_info()
    B, K = thetas.shape
    assert c.shape == e.shape == s.shape == (B,) and g.shape == (B, K)
    assert all(np.all(np.isfinite(a)) for a in (c, g, e, s)) and np.all(s >= 0.0)
    assert (info["B"], info["K"], info["mode"]) == (B, K, int(omega is None)), info
    assert np.abs(c - (we * e + ws * s)).max() <= 1e-14 * max(1.0, float(np.abs(c).max()))
    return c, g, e, s, info


def _omegas(case, thetas, seed):
    """one omega per row: the row's own energy shifted by up to +-0.5 (the checker's energy: nothing of the device's)"""
    shift = np.random.default_rng(seed).uniform(-0.5, 0.5, len(thetas))
    return np.array([case.want(t)[0] for t in thetas]) + shift


_WANT = {}


def _want(case, theta, omega, we, ws):
    key = (id(case), np.ascontiguousarray(theta, np.float64).tobytes(), omega, we, ws)
    if key not in _WANT:
        _WANT[key] = sp.case_want(case, theta, omega, we, ws)
    return _WANT[key]


def _against_checker(case, thetas, omega, out, rows, we=WE, ws=WS, what=""):
    c, g, e, s = out[:4]
    tol = sp.bound_checker(case, omega, we, ws)
    for b in rows:
        om = None if omega is None else float(np.broadcast_to(omega, (len(thetas),))[b])
        cw, gw, ew, sw = _want(case, thetas[b], om, we, ws)
        dcost, de, ds, dg = abs(c[b] - cw), abs(e[b] - ew), abs(s[b] - sw), float(np.abs(g[b] - gw).max(initial=0.0))
        print(f"   {what} row {b} {'variance' if omega is None else 'omega given'}: |dC| {dcost:.3e} |dE| {de:.3e} |dS| {ds:.3e} max|dg| {dg:.3e} "
              f"bound {tol:.3e}; S {sw:.4e} max|g| {np.abs(gw).max(initial=0.0):.4f}")
        assert dcost <= tol and de <= tol and ds <= tol and dg <= tol


def _against_single_rows(sv, case, thetas, omega, out, rows, we=WE, ws=WS):
    c, g, e, s = out[:4]
    tol = sp.bound_single(case, omega, we, ws)
    for b in rows:
        om = None if omega is None else np.broadcast_to(omega, (len(thetas),))[b:b + 1]
        c1, g1, e1, s1 = sv.spread_gradient_batch(thetas[b:b + 1], om, we, ws)
        assert abs(c1[0] - c[b]) <= tol and abs(e1[0] - e[b]) <= tol and abs(s1[0] - s[b]) <= tol
        assert np.abs(g1[0] - g[b]).max(initial=0.0) <= tol


def _sizes(sv, info, K):
    """(slots, ntab, nops, npairs, K) of the handle's compact program, the table entries from the LDS bytes of this launch"""
    pi = sv.program_info()
    m, nops, npairs = gc.slots(info["support"]), pi["sp_ops"], pi["sp_pairs"]
    stride, rest = divmod(info["lds_bytes"] - (nops * 16 + npairs * 4 if info["form"] == 1 else 0), info["waves"])
    assert rest == 0 and stride % 16 == 0 and pi["support"] == info["support"], info
    ntab = (stride - 3 * ((m + 1) & ~1) * 8 - ((K + 1) & ~1) * 8) // 24
    assert sp.wave_stride(m, ntab, K) == stride, (info, pi, ntab)
    return m, ntab, nops, npairs, K


def _path1(sv, info, K, B, mode, waves=0, workgroups=0, sizes=None):
    sizes = _sizes(sv, info, K) if sizes is None else sizes
    sp.check_info(info, sizes, B, mode, waves=waves, workgroups=workgroups)
    return sizes


def _path2(info, why):
    assert info["path"] == 2 and info["why"] == why and info["launches"] == 6 * info["B"], info
    assert not any(info[k] for k in ("form", "waves", "workgroups", "lds_bytes", "support", "launch_us", "copy_back_us")), info


def _both_modes(sv, case, thetas, seed, rows_checker, rows_single, what, **plan):
    """a path-1 batch whose last row repeats row 0, in both modes with the mixed weights -> the sizes of the compact program"""
    B = len(thetas)
    sizes = plan.pop("sizes", None)
    for omega in (None, _omegas(case, thetas, seed)):
        if omega is not None:
            omega[B - 1] = omega[0]
        out = _call(sv, thetas, omega)
        c, g, e, s, info = out
        sizes = _path1(sv, info, case.K, B, int(omega is None), sizes=sizes, **plan)
        assert _same_bits(e[0], e[B - 1]) and _same_bits(s[0], s[B - 1]) and _same_bits(c[0], c[B - 1])
        _against_checker(case, thetas, omega, out, rows_checker, what=what)
        _against_single_rows(sv, case, thetas, omega, out, rows_single)
    return sizes, info


# ---- path 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["two_states", "per_rotation_9", "h4"])
def test_small_supports(SV, h4, which):
    """m = 2, m = 128 (the whole 7-qubit register) and H4 (m = 36): B = 5 against the checker and single-row calls in both modes; equal
    rows give equal bits in energies and spreads"""
    case = {"two_states": lambda: gc.two_states()[0], "per_rotation_9": lambda: gc.per_rotation(9), "h4": lambda: h4}[which]()
    thetas = np.random.default_rng(len(which)).uniform(-0.5, 0.5, (5, case.K))
    thetas[4] = thetas[0]
    with SV(case.n) as sv:
        case.load(sv) if which != "h4" else (sv.set_hamiltonian(case.ham), sv.set_ucc_program(case.gens, case.hf))
        _, info = _both_modes(sv, case, thetas, 11, range(4), [0, 2, 4], which)
        e, var = sv.energy_variance(thetas[1])
    print(f"{which}: {info}")
    assert info["support"] == {"two_states": 2, "per_rotation_9": 128, "h4": 36}[which]
    cw, gw, ew, sw = _want(case, thetas[1], None, WE, WS)
    assert abs(e - ew) <= sp.bound_checker(case, None, 0.0, 1.0) and abs(var - sw) <= sp.bound_checker(case, None, 0.0, 1.0)


@pytest.fixture(scope="module")
def lih_rows(lih):
    return np.random.default_rng(12).uniform(-0.2, 0.2, (41, lih.K))


@pytest.mark.parametrize("nw", [1, 2, 4, 8])
def test_lih_every_wave_count(SV, lih, lih_rows, nw):
    """LiH UCCSD (m = 225 in 256 slots, K = 92) under "grad_batch_waves" = nw: B = nw + 1, and B = 5 nw + 1 on two workgroups — idle
    waves, second and third trips"""
    with SV(lih.n) as sv:
        sv.set_option("grad_batch_waves", nw)
        sv.set_hamiltonian(lih.ham)
        sv.set_ucc_program(lih.gens, lih.hf)
        sizes = None
        for B, wgs in ((nw + 1, 0), (5 * nw + 1, 2)):
            sv.set_option("grad_batch_workgroups", wgs)
            thetas = lih_rows[:B].copy()
            thetas[B - 1] = thetas[0]
            sizes, info = _both_modes(sv, lih, thetas, 13, [0, 1] if wgs == 0 else [1], [0, B // 2, B - 1], f"LiH nw {nw} B {B}",
                                      waves=nw, workgroups=wgs, sizes=sizes)
            print(f"LiH nw = {nw} B = {B}: {info}")
            assert info["support"] == 225 and sizes[0] == 256 and info["waves"] == nw
            assert info["workgroups"] == (2 if wgs else -(-B // nw))


def test_4096_states(SV):
    """y_program(14), m = 4096 on 12 qubits: one three-array region is 96 KiB — one wave per workgroup, one workgroup per CU"""
    case, sizes = gc.y_program(14), gc.y_sizes(14)
    thetas = np.random.default_rng(14).uniform(-0.7, 0.7, (3, case.K))
    thetas[2] = thetas[0]
    with SV(case.n) as sv:
        case.load(sv)
        _, info = _both_modes(sv, case, thetas, 15, [1], [0, 2], "y_program(14)", sizes=sizes)
    print(f"y_program(14): {info}")
    want = sp.plan(*sizes, 3)
    assert (want["nw"], want["stage"], want["per_cu"]) == (1, True, 1) and info["support"] == 4096 and info["waves"] == 1 and info["form"] == 1
    assert info["lds_bytes"] == sp.wave_stride(4096, 14, gc.Y_K) + sizes[2] * 16 + sizes[3] * 4 and sp.wave_stride(4096, 14, gc.Y_K) >= 96 * 1024


@pytest.mark.parametrize("which", ["two_states", "h4", "lih"])
def test_energy_weight_alone_is_the_batched_gradient(SV, h4, lih, which):
    """w = (1, 0): costs and energies equal energy_gradient_batch's to the bit (the same summation order), gradients within the
    same-handle bound"""
    case = {"two_states": lambda: gc.two_states()[0], "h4": lambda: h4, "lih": lambda: lih}[which]()
    thetas = np.random.default_rng(70).uniform(-0.3, 0.3, (7, case.K))
    with SV(case.n) as sv:
        sv.set_hamiltonian(case.ham)
        sv.set_rotation_program(case.rx, case.rz, case.rc, case.pidx, case.K, case.hf, phi0=case.phi0)
        e0, g0 = sv.energy_gradient_batch(thetas)
        assert sv.gradient_batch_info()["path"] == 1
        for omega in (None, _omegas(case, thetas, 71)):
            c, g, e, s, info = _call(sv, thetas, omega, 1.0, 0.0)
            assert info["path"] == 1 and _same_bits(c, e0) and _same_bits(e, e0)
            dg = np.abs(g - g0).max()
            print(f"{which}: max |dg| {dg:.3e} bound {sp.bound_single(case, omega, 1.0, 0.0):.3e}")
            assert dg <= sp.bound_single(case, omega, 1.0, 0.0)


def test_the_lds_boundary(SV):
    """the last y_program(R) whose three-array region fits 150 KiB runs on path 1, the next one falls to path 2 with reason 2 (the
    batched gradient still takes its own path 1 there); both against the checker"""
    last, first = sp.y_lds_boundary()
    for R in (last, first):
        case, sizes = gc.y_program(R), gc.y_sizes(R)
        thetas = np.random.default_rng(R).uniform(-0.7, 0.7, (2, case.K))
        with SV(case.n) as sv:
            case.load(sv)
            out = _call(sv, thetas, None)
            info = out[4]
            print(f"R = {R}: {info}")
            if R == last:
                _path1(sv, info, case.K, 2, 1, sizes=sizes)
                assert info["lds_bytes"] <= 150 * 1024 < info["lds_bytes"] + 24
            else:
                _path2(info, 2)
                sv.energy_gradient_batch(thetas)
                assert sv.gradient_batch_info()["path"] == 1
        _against_checker(case, thetas, None, out, [1], what=f"R {R}")


# ---- the traps: what the compact program drops ------------------------------------------------------------------------------------------
def test_a_hamiltonian_that_leaks_from_the_support(SV):
    """per_rotation(3) with 0.3 X on index bit 5 beside its own Hamiltonian: the compact program's entries never see the term, <H> is
    right without it, ||H psi||^2 is not — path 2 with reason 3, S the checker's, 0.09 above the support-restricted value"""
    closed, leaky = sp.leak_case()
    thetas = np.random.default_rng(5).uniform(-0.6, 0.6, (3, closed.K))
    with SV(closed.n) as sv:
        closed.load(sv)
        inside = _call(sv, thetas, None)
        _path1(sv, inside[4], closed.K, 3, 1)
        leaky.load(sv)
        for omega in (None, _omegas(leaky, thetas, 6)):
            out = _call(sv, thetas, omega)
            _path2(out[4], 3)
            _against_checker(leaky, thetas, omega, out, range(3), what="leak")
            if omega is None:
                print("S beside the restricted value:", out[3] - inside[3])
                assert np.abs(out[3] - inside[3] - sp.LEAK_COEFF ** 2).max() <= sp.bound_checker(leaky, None, 0.0, 1.0)
        sv.energy_gradient_batch(thetas)
        assert sv.gradient_batch_info()["path"] == 1          # <H> and its gradient keep the compact path: exact there


def test_a_hamiltonian_with_an_odd_y_term(SV):
    """the same program with 0.2 Y on index bit 1, inside the support: path 2 with reason 4, S the checker's"""
    closed, oddy = sp.odd_y_case()
    thetas = np.random.default_rng(7).uniform(-0.6, 0.6, (3, closed.K))
    with SV(closed.n) as sv:
        oddy.load(sv)
        for omega in (None, _omegas(oddy, thetas, 8)):
            out = _call(sv, thetas, omega)
            _path2(out[4], 4)
            _against_checker(oddy, thetas, omega, out, range(3), what="odd Y")
            if omega is None:      # what a kernel that trusts the restricted entries would return: the closed Hamiltonian's variance
                assert np.all(out[3] - np.array([sp.case_want(closed, t)[3] for t in thetas]) > 1e-3)


# ---- path 2 ------------------------------------------------------------------------------------------------------------------------------
def test_path_2_forced_on_h4(SV, h4):
    """"force_path" 2: the streaming rows meet the checker and path 1's results, and are bit-identical from call to call"""
    thetas = np.random.default_rng(9).uniform(-0.3, 0.3, (3, h4.K))
    with SV(h4.n) as sv:
        sv.set_hamiltonian(h4.ham)
        sv.set_ucc_program(h4.gens, h4.hf)
        one = _call(sv, thetas, None)
        assert one[4]["path"] == 1
    with SV(h4.n) as sv:
        sv.set_option("force_path", 2)
        sv.set_hamiltonian(h4.ham)
        sv.set_ucc_program(h4.gens, h4.hf)
        for omega in (None, _omegas(h4, thetas, 10)):
            out = _call(sv, thetas, omega)
            _path2(out[4], 1)
            again = _call(sv, thetas, omega)
            assert all(_same_bits(a, b) for a, b in zip(out[:4], again[:4]))
            _against_checker(h4, thetas, omega, out, range(3), what="H4 streaming")
            _against_single_rows(sv, h4, thetas, omega, out, [0, 2])
            if omega is None:
                tol = sp.bound_checker(h4, None, WE, WS)
                assert all(np.abs(a - b).max() <= tol for a, b in zip(out[:4], one[:4]))


def test_path_2_literal_gate_list(SV):
    """the reference's QUCCSD templates as a literal gate list, Clifford frame as the library chooses it: no refusal, the checker through
    ``metric_cases.gate_tangents``"""
    from tests.util import quccsd_like_gates
    n, hf = 8, 0b11010010
    rng = np.random.default_rng(8200)
    gates, K = quccsd_like_gates(rng, n, 3, 2, extra_random=6)
    hx, hz, hc = hessian_cases.random_real_hamiltonian(n, 16, 23)
    ham = hessian_cases.hamiltonian_object(n, hx, hz, hc, 0.1)

    class G:
        h = (hx, hz, hc, 0.1)
        C = max(sum(0.5 * abs(g[2]) for g in gates if g[4] == k) for k in range(K))

    thetas = rng.uniform(-0.7, 0.7, (2, K))
    with SV(n) as sv:
        sv.set_hamiltonian(ham)
        sv.set_gate_program(gates, K, hf)
        for omega in (None, np.array([0.2, -0.4])):
            c, g, e, s, info = _call(sv, thetas, omega)
            _path2(info, 1)
            tol = sp.bound_checker(G, omega, WE, WS)
            for b in range(2):
                cw, gw, ew, sw = sp.spread_gradient_gates(n, hf, gates, thetas[b], hx, hz, hc, 0.1, None if omega is None else omega[b], WE, WS)
                print(f"   gate list row {b}: |dC| {abs(c[b] - cw):.3e} |dS| {abs(s[b] - sw):.3e} max|dg| {np.abs(g[b] - gw).max():.3e} bound {tol:.3e}")
                assert abs(c[b] - cw) <= tol and abs(e[b] - ew) <= tol and abs(s[b] - sw) <= tol and np.abs(g[b] - gw).max() <= tol


def test_path_2_beside_the_sector_tables(SV):
    """a program whose single gradient runs on the sector tables: the spread call streams, meets the checker, and the single call still
    reports its sector forms afterwards"""
    from tests import sector_cases as sc
    case = sc.molecule(7, 2)
    theta = np.array(case.thetas(2)[:1])
    const = float(np.real(case.ham.constant_coeff or 0.0))

    class G:
        h = (case.hx, case.hz, case.hc, const)
        C = hessian_cases.coefficient_sum(case.rc, case.pidx, case.K)

    with SV(case.n) as sv:
        for k, v in {"force_path": 2, "sector_min_qubits": 8}.items():
            sv.set_option(k, v)
        sv.set_hamiltonian(case.ham)
        sv.set_ucc_program(case.gens, case.hf)
        es, gs = sv.energy_gradient(theta[0])
        forms = sv.sector_forms()
        assert forms
        c, g, e, s, info = _call(sv, theta, None)
        _path2(info, 1)
        es2, gs2 = sv.energy_gradient(theta[0])
        assert sv.sector_forms() == forms and abs(es - es2) <= 1e-12 * case.bound and np.abs(gs - gs2).max() <= 1e-12 * case.bound
    assert abs(e[0] - es) <= 1e-10 * case.bound
    cw, gw, ew, sw = sp.spread_gradient(case.n, case.hf, case.rx, case.rz, case.rc, case.pidx, theta[0], case.hx, case.hz, case.hc, const,
                                        None, None, WE, WS)
    tol = sp.bound_checker(G, None, WE, WS)
    print(f"sector case: |dC| {abs(c[0] - cw):.3e} |dS| {abs(s[0] - sw):.3e} max|dg| {np.abs(g[0] - gw).max():.3e} bound {tol:.3e}; S {sw:.4e}")
    assert abs(c[0] - cw) <= tol and abs(e[0] - ew) <= tol and abs(s[0] - sw) <= tol and np.abs(g[0] - gw).max() <= tol


# ---- contract ----------------------------------------------------------------------------------------------------------------------------
SENTINEL = -7.25
INVALID, STATE = -1, -5


def _raw(sv, B, theta, K, omega, we, ws, costs, grads, energies, spreads):
    rc = sv._L.ovqe_spread_gradient_batch(sv._h, B, theta, K, omega, we, ws, costs, grads, energies, spreads)
    return rc, (sv._L.ovqe_last_error(sv._h) or b"").decode()


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("mode", [0, 1])
def test_bounds_of_the_six_arrays(SV, h4, path, mode):
    """theta and omega with NaN tails, the four outputs with sentinel tails: finite results, untouched sentinels"""
    B, K = 5, h4.K
    rows = np.random.default_rng(15).uniform(-0.3, 0.3, (B, K))
    theta = np.concatenate([rows.reshape(-1), np.full(3 * K, np.nan)])
    om = _omegas(h4, rows, 16)
    omega = np.concatenate([om, np.full(8, np.nan)]) if mode == 0 else None
    costs, energies, spreads, grads = np.full(B + 16, SENTINEL), np.full(B + 16, SENTINEL), np.full(B + 16, SENTINEL), np.full(B * K + 64, SENTINEL)
    with SV(h4.n) as sv:
        sv.set_option("force_path", 2 if path == 2 else 0)
        sv.set_hamiltonian(h4.ham)
        sv.set_ucc_program(h4.gens, h4.hf)
        rc, msg = _raw(sv, B, theta, K, omega, WE, WS, costs, grads, energies, spreads)
        assert rc == 0, msg
        assert sv.spread_info()["path"] == path and sv.spread_info()["mode"] == mode
        c, g, e, s = sv.spread_gradient_batch(rows, om if mode == 0 else None, WE, WS)
    for arr, used in ((costs, B), (energies, B), (spreads, B), (grads, B * K)):
        assert np.all(np.isfinite(arr[:used])) and np.all(arr[used:] == SENTINEL)
    tol = sp.bound_single(h4, om if mode == 0 else None, WE, WS)
    assert np.abs(costs[:B] - c).max() <= tol and np.abs(spreads[:B] - s).max() <= tol and np.abs(grads[:B * K] - g.reshape(-1)).max() <= tol


def test_refusals_and_the_empty_batch(SV):
    n, hf, rx, rz, rc, pidx, phi0, K = metric_cases.tied_program()
    case = gc.Case(n, hf, rx, rz, rc, pidx, K, phi0=phi0, nterms=24, seed=17)
    theta, om = np.zeros(2 * K), np.zeros(2)
    c, e, s, g = np.full(2, SENTINEL), np.full(2, SENTINEL), np.full(2, SENTINEL), np.full(2 * K, SENTINEL)

    def refused(sv, code, text, *args):
        rc, msg = _raw(sv, *args)
        assert rc == code and text in msg, (rc, msg)

    with SV(n) as sv:
        info = (ctypes.c_int64 * 13)(*([7] * 13))
        assert sv._L.ovqe_spread_info(sv._h, info, 13) == 0 and not any(info)          # zeros before the first call
        refused(sv, STATE, "no program set", 2, theta, K, om, WE, WS, c, g, e, s)
        sv.set_rotation_program(rx, rz, rc, pidx, K, hf, phi0=phi0)
        refused(sv, STATE, "no Hamiltonian set", 2, theta, K, om, WE, WS, c, g, e, s)
        sv.set_hamiltonian(case.ham)
        refused(sv, INVALID, "K does not match", 2, theta, K - 1, om, WE, WS, c, g, e, s)
        refused(sv, INVALID, "B is negative", -1, theta, K, om, WE, WS, c, g, e, s)
        refused(sv, INVALID, "theta is NULL", 2, None, K, om, WE, WS, c, g, e, s)
        refused(sv, INVALID, "costs is NULL", 2, theta, K, om, WE, WS, None, g, e, s)
        refused(sv, INVALID, "grads is NULL", 2, theta, K, om, WE, WS, c, None, e, s)
        for bad in (np.nan, np.inf, -np.inf):
            refused(sv, INVALID, "weights must be finite", 2, theta, K, om, bad, WS, c, g, e, s)
            refused(sv, INVALID, "weights must be finite", 2, theta, K, None, WE, bad, c, g, e, s)
            refused(sv, INVALID, "omega[1] is not finite", 2, theta, K, np.array([0.0, bad]), WE, WS, c, g, e, s)
        sv.set_option("real_state", 1)
        refused(sv, STATE, "real_state", 2, theta, K, om, WE, WS, c, g, e, s)
        sv.set_option("real_state", 0)
        assert sv._L.ovqe_spread_info(sv._h, info, 13) == 0 and not any(info)          # refused calls leave no figures
        assert all(np.all(a == SENTINEL) for a in (c, g, e, s))
        # B = 0: OVQE_OK, nothing touched, NULL arrays allowed
        assert _raw(sv, 0, None, K, None, WE, WS, None, None, None, None)[0] == 0 and _raw(sv, 0, theta, K, om, WE, WS, c, g, e, s)[0] == 0
        assert all(np.all(a == SENTINEL) for a in (c, g, e, s))
        assert sv._L.ovqe_spread_info(sv._h, info, 13) == 0 and not any(info)
        out = sv.spread_gradient_batch(np.zeros((0, K)))
        assert [a.shape for a in out] == [(0,), (0, K), (0,), (0,)]
        # energies and spreads may be NULL, each alone
        assert _raw(sv, 2, theta, K, om, WE, WS, c, g, None, None)[0] == 0 and np.all(c != SENTINEL) and np.all(e == SENTINEL) and np.all(s == SENTINEL)
        assert _raw(sv, 2, theta, K, None, WE, WS, c, g, None, s)[0] == 0 and np.all(e == SENTINEL) and np.all(s != SENTINEL)
        assert sv._L.ovqe_spread_info(sv._h, info, 13) == 0 and list(info)[:4] == [2, 2, K, 1] and info[10] == 1
        assert sv._L.ovqe_spread_info(sv._h, info, -1) == INVALID and sv._L.ovqe_spread_info(sv._h, None, 13) == INVALID
        for bad in (np.zeros(K), np.zeros((2, K + 1)), np.zeros((1, 2, K))):
            with pytest.raises(ValueError):
                sv.spread_gradient_batch(bad)
    with SV(n - 1, n_global=1, shard_index=0) as shard:
        rc, msg = _raw(shard, 2, theta, K, om, WE, WS, c, g, e, s)
        assert rc != 0 and rc == shard._L.ovqe_energy_gradient_batch(shard._h, 2, theta, K, e, g), (rc, msg)


def test_null_outputs_on_the_compact_path(SV, h4):
    thetas = np.random.default_rng(31).uniform(-0.3, 0.3, (3, h4.K))
    c, g, e, s = np.full(3, SENTINEL), np.full(3 * h4.K, SENTINEL), np.full(3, SENTINEL), np.full(3, SENTINEL)
    with SV(h4.n) as sv:
        sv.set_hamiltonian(h4.ham)
        sv.set_ucc_program(h4.gens, h4.hf)
        full = sv.spread_gradient_batch(thetas, None, WE, WS)
        assert _raw(sv, 3, thetas.reshape(-1), h4.K, None, WE, WS, c, g, None, None)[0] == 0 and sv.spread_info()["path"] == 1
        assert np.all(e == SENTINEL) and np.all(s == SENTINEL) and _same_bits(c, full[0])
        assert _raw(sv, 3, thetas.reshape(-1), h4.K, None, WE, WS, c, g, e, None)[0] == 0 and _same_bits(e, full[2]) and np.all(s == SENTINEL)
        assert _raw(sv, 3, thetas.reshape(-1), h4.K, None, WE, WS, c, g, None, s)[0] == 0 and _same_bits(s, full[3])


@pytest.mark.parametrize("path", [0, 2])
def test_neighbours_untouched(SV, h4, path):
    """cached tables stay valid: energy and energy_batch before and after a spread call to the bit, energy_gradient within 1e-13, the
    compact forms the handle reports unchanged"""
    theta = np.random.default_rng(9).uniform(-0.3, 0.3, h4.K)
    thetas = np.random.default_rng(10).uniform(-0.3, 0.3, (7, h4.K))
    with SV(h4.n) as sv:
        sv.set_option("force_path", path)
        sv.set_hamiltonian(h4.ham)
        sv.set_ucc_program(h4.gens, h4.hf)
        e0 = sv.energy(theta)
        b0 = sv.energy_batch(np.tile(theta, (3, 1)))
        ge0 = sv.energy_gradient(theta)
        forms, geometries = sv.sparse_forms(), sv.sparse_geometries()
        for omega in (None, -1.9):
            sv.spread_gradient_batch(thetas, omega, WE, WS)
            assert sv.spread_info()["path"] == (2 if path == 2 else 1)
        if path == 0:
            assert (sv.sparse_forms(), sv.sparse_geometries()) == (forms, geometries)
        e1 = sv.energy(theta)
        b1 = sv.energy_batch(np.tile(theta, (3, 1)))
        ge1 = sv.energy_gradient(theta)
    assert np.float64(e0).view(np.int64) == np.float64(e1).view(np.int64)
    assert np.array_equal(b0.view(np.int64), b1.view(np.int64))
    assert abs(ge0[0] - ge1[0]) <= 1e-13 * h4.h1 and np.abs(ge0[1] - ge1[1]).max() <= 1e-13 * h4.h1


# ---- the driver --------------------------------------------------------------------------------------------------------------------------
def test_folded_spectrum_on_lih(SV, lih):
    """LiH, omega = E_FCI + 0.02, one start from theta = 0: path 1; the Weinstein statement against the sector's Lanczos ground state —
    an eigenvalue lies within sqrt(variance) of the returned energy, and the energy is not below E_FCI.  No convergence target: the
    UCCSD ansatz does not hold the FCI state, how near it comes is printed"""
    with SV(lih.n) as sv:
        sv.set_hamiltonian(lih.ham)
        sv.init_basis(lih.hf)
        e_fci = sv.sector_ground_state(tol=1e-12)[0]
        sv.set_ucc_program(lih.gens, lih.hf)
        (state,) = excited.folded_spectrum(sv, [e_fci + 0.02], starts=1)
        info = sv.spread_info()
        e, var = sv.energy_variance(state["theta"])
    res = state["result"]
    print(f"LiH: FCI {e_fci:.10f}; folded-spectrum energy {state['energy']:.10f} spread {state['spread']:.6e} variance {state['variance']:.6e} "
          f"iterations {res.nit} calls {res.ncalls} status {res.status}; {info}")
    assert info["path"] == 1 and info["mode"] == 1 and info["support"] == 225
    assert np.all(np.diff(res.energies) <= 0.0) and res.energies[-1] < res.energies[0]
    assert _same_bits(e, state["energy"]) and _same_bits(var, state["variance"])
    # Weinstein, against the one eigenvalue known here: E_FCI is the lowest level of the sector the state lives in, and the level omega
    # was placed beside
    assert state["energy"] >= e_fci - 1e-9 and state["variance"] >= 0.0
    assert state["energy"] - e_fci <= np.sqrt(state["variance"]) + 1e-9
