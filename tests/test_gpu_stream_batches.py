"""GPU tests of the three batched gradient calls where their compact path ends — ovqe_energy_gradient_batch, ovqe_deflated_gradient_batch,
ovqe_spread_gradient_batch on registers above 16 qubits, where every row goes through the streaming kernels (abi_gradbatch.inc,
abi_deflate.inc, abi_spread.inc; apply_hamiltonian in tile_host.inc; k_deflate_dots / k_deflate_axpy in sv_deflate.hpp; k_dot, k_scale,
k_axpy_real, k_reduce in sv_kernels.hpp).  Cases and the constants they are derived from: tests/stream_cases.py.

Checkers: ``oracle.masks.ucc_energy_gradient``, ``deflation_cases.deflated_gradient``, ``spread_cases.spread_gradient`` on the dense complex
register.  Bounds: ``gradbatch_cases.bound_checker`` / ``bound_single`` (1e-10 / 1e-12 ||H||_1 max(1, C)), their deflation and spread
counterparts with the larger operator norms, ``deflation_cases.bound_overlap`` (1e-12 ||phi_j||).  The checker is the cost of these
tests (seconds per row at 19 and 20 qubits): a test has at most two checker rows at 20 qubits and three at 19, every other row is
compared with another call on the same handle.

What the header does not promise, and what is pinned instead: the state buffer after a batched call is unspecified — ovqe_energy and
ovqe_energy_gradient before and after the calls are compared; path 2 of the deflated call with no vector held equals
ovqe_energy_gradient_batch within the same-handle bound (costs equal energies to the bit, as promised; whether the energies of the two
calls agree to the bit is printed)."""
import numpy as np
import pytest

from tests import deflation_cases as dc
from tests import gradbatch_cases as gc
from tests import spread_cases as sp
from tests import stream_cases as st

pytestmark = pytest.mark.gpu

WE, WS = 0.3, 1.0     # the mixed weights of the spread calls
GRAD_FORMS = {"grad_wg", "grad_staged", "grad_plain"}


@pytest.fixture(scope="module")
def SV(gpu_lib):
    from openvqe_amd.backend import Statevector
    return Statevector


class Held:
    """the vectors a handle holds, as the checker sees them: read back from the buffer that was pushed"""

    def __init__(self):
        self.vectors, self.betas = [], []

    def push_state(self, sv, beta):
        before = sv.get_state()
        sv.deflation_push(beta)
        assert np.array_equal(sv.get_state().view(np.int64), before.view(np.int64))     # the buffer is only read
        self.vectors.append(before)
        self.betas.append(float(beta))

    def push_set(self, sv, vset):
        for kind, v, beta in vset:
            sv.prepare_state(v) if kind == "ansatz" else sv.set_state(v)
            self.push_state(sv, beta)

    def truncate(self, sv, count):
        sv.deflation_truncate(count)
        del self.vectors[count:], self.betas[count:]


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _all_same_bits(one, two):
    return all(_same_bits(a, b) for a, b in zip(one[:4], two[:4]))


def _dev(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max(initial=0.0))


# ---- the three calls, with the checks every result gets ---------------------------------------------------------------------------------
def _plain(sv, thetas):
    """-> (energies, grads, energies, None, info): the layout of the other two calls, costs = energies"""
    thetas = np.ascontiguousarray(thetas, np.float64)
    e, g = sv.energy_gradient_batch(thetas)
    info = sv.gradient_batch_info()
    assert e.shape == (len(thetas),) and g.shape == thetas.shape and np.all(np.isfinite(e)) and np.all(np.isfinite(g))
    assert (info["B"], info["K"]) == thetas.shape, info
    return e, g, e, None, info


def _deflated(sv, thetas, held):
    thetas = np.ascontiguousarray(thetas, np.float64)
    c, g, e, o = sv.deflated_gradient_batch(thetas)
    info = sv.deflation_info()
    B, K = thetas.shape
    J = len(held.vectors)
    assert c.shape == e.shape == (B,) and g.shape == (B, K) and o.shape == (B, J) and o.dtype == np.complex128
    assert all(np.all(np.isfinite(a)) for a in (c, g, e, o.view(np.float64)))
    assert (info["B"], info["K"], info["J"]) == (B, K, J) and sv.deflation_count() == J, info
    pen = np.array([sum(b * abs(x) ** 2 for b, x in zip(held.betas, row)) for row in o]).reshape(B)
    assert np.abs(c - e - pen).max() <= 1e-13 * dc.weight(1.0, held.vectors, held.betas)     # cost = energy + penalty of the returned overlaps
    return c, g, e, o, info


def _spread(sv, thetas, omega=None, we=WE, ws=WS):
    thetas = np.ascontiguousarray(thetas, np.float64)
    c, g, e, s = sv.spread_gradient_batch(thetas, omega, we, ws)
    info = sv.spread_info()
    B, K = thetas.shape
    assert c.shape == e.shape == s.shape == (B,) and g.shape == (B, K)
    assert all(np.all(np.isfinite(a)) for a in (c, g, e, s)) and np.all(s >= 0.0)
    assert (info["B"], info["K"], info["mode"]) == (B, K, int(omega is None)), info
    assert np.abs(c - (we * e + ws * s)).max() <= 1e-14 * max(1.0, float(np.abs(c).max()))
    return c, g, e, s, info


def _plain_path2(info):
    assert info["path"] == 2 and not any(info[k] for k in ("launches", "form", "waves", "workgroups", "lds_bytes", "support")), info


def _deflated_path2(info):
    assert info["path"] == 2 and info["launches"] == st.deflation_launches(info["B"], info["J"]), info
    assert not any(info[k] for k in ("rows", "form", "waves", "workgroups", "lds_bytes", "support", "gather_launches")), info


def _spread_path2(info, why=1):
    assert info["path"] == 2 and info["why"] == why and info["launches"] == 6 * info["B"], info
    assert not any(info[k] for k in ("form", "waves", "workgroups", "lds_bytes", "support", "launch_us", "copy_back_us")), info


# ---- comparisons --------------------------------------------------------------------------------------------------------------------------
def _plain_checker(case, thetas, out, rows, what):
    tol = case.tol_checker()
    for b in rows:
        ew, gw = case.want(thetas[b])
        de, dg = abs(out[0][b] - ew), _dev(out[1][b], gw)
        print(f"   {what} row {b} against the checker: |dE| {de:.3e} max|dg| {dg:.3e} bound {tol:.3e}; E {ew:.6f} max|g| {np.abs(gw).max():.4f}")
        assert de <= tol and dg <= tol


def _plain_single(sv, case, thetas, out, rows, what):
    tol = case.tol_single()
    worst = 0.0
    for b in rows:
        e1, g1 = sv.energy_gradient(thetas[b])
        worst = max(worst, abs(e1 - out[0][b]), _dev(g1, out[1][b]))
    print(f"   {what} rows {list(rows)} against energy_gradient: {worst:.3e} bound {tol:.3e}")
    assert worst <= tol


def _deflated_checker(case, held, thetas, out, rows, what):
    c, g, e, o = out[:4]
    tol = dc.bound_checker(case.h1, case.C, held.vectors, held.betas)
    for b in rows:
        cw, gw, ew, ow = dc.case_want(case, thetas[b], held.vectors, held.betas)
        dcost, de, dg = abs(c[b] - cw), abs(e[b] - ew), _dev(g[b], gw)
        do = np.abs(o[b] - ow) if len(ow) else np.zeros(0)
        print(f"   {what} row {b} against the checker: |dC| {dcost:.3e} |dE| {de:.3e} max|dg| {dg:.3e} bound {tol:.3e}; max overlap deviation "
              f"{do.max(initial=0.0):.2e} of {len(ow)} bound {dc.bound_overlap(held.vectors[0]) if len(ow) else 0.0:.1e}; penalty {cw - ew:.4f}")
        assert dcost <= tol and de <= tol and dg <= tol
        assert all(x <= dc.bound_overlap(v) for x, v in zip(do, held.vectors))     # every slot, both parts


def _deflated_single(sv, case, held, thetas, out, rows, what):
    c, g, e, o = out[:4]
    tol = dc.bound_single(case.h1, case.C, held.vectors, held.betas)
    worst, worst_o = 0.0, 0.0
    for b in rows:
        c1, g1, e1, o1 = sv.deflated_gradient_batch(thetas[b:b + 1])
        worst = max(worst, abs(c1[0] - c[b]), abs(e1[0] - e[b]), _dev(g1[0], g[b]))
        worst_o = max(worst_o, _dev(o1[0], o[b]))
        assert all(abs(x - y) <= dc.bound_overlap(v) for x, y, v in zip(o1[0], o[b], held.vectors))
    print(f"   {what} rows {list(rows)} against one-row calls: {worst:.3e} bound {tol:.3e}; overlaps {worst_o:.2e}")
    assert worst <= tol


def _row_omega(omega, b, B):
    return None if omega is None else float(np.broadcast_to(omega, (B,))[b])


def _spread_checker(case, thetas, omega, out, rows, what, we=WE, ws=WS):
    c, g, e, s = out[:4]
    tol = sp.bound_checker(case, omega, we, ws)
    for b in rows:
        cw, gw, ew, sw = sp.case_want(case, thetas[b], _row_omega(omega, b, len(thetas)), we, ws)
        dcost, de, ds, dg = abs(c[b] - cw), abs(e[b] - ew), abs(s[b] - sw), _dev(g[b], gw)
        print(f"   {what} row {b} {'variance' if omega is None else 'omega given'} against the checker: |dC| {dcost:.3e} |dE| {de:.3e} |dS| {ds:.3e} "
              f"max|dg| {dg:.3e} bound {tol:.3e}; S {sw:.4e} max|g| {np.abs(gw).max():.4f}")
        assert dcost <= tol and de <= tol and ds <= tol and dg <= tol


def _spread_single(sv, case, thetas, omega, out, rows, what, we=WE, ws=WS):
    c, g, e, s = out[:4]
    tol = sp.bound_single(case, omega, we, ws)
    worst = 0.0
    for b in rows:
        om = None if omega is None else np.broadcast_to(omega, (len(thetas),))[b:b + 1]
        c1, g1, e1, s1 = sv.spread_gradient_batch(thetas[b:b + 1], om, we, ws)
        worst = max(worst, abs(c1[0] - c[b]), abs(e1[0] - e[b]), abs(s1[0] - s[b]), _dev(g1[0], g[b]))
    print(f"   {what} rows {list(rows)} against one-row calls: {worst:.3e} bound {tol:.3e}")
    assert worst <= tol


def _apply_cover_of_the_handle(sv, case, what):
    """the precondition of the tiled H psi: at least two sweeps, nothing untiled — by the restated rule (held to sv_cover_host.hpp on the
    CPU), and by ovqe_program_info where its entries describe this cover: they are the complex register's (h->ham, the cover
    apply_hamiltonian builds on its first use) unless the real-amplitude stream keeps a cover of its own ("real_stream" of the info)"""
    sweeps, rest = st.apply_cover(case.n, case.h[0])
    pi = sv.program_info()
    print(f"   {what}: cover restated {len(sweeps)} sweeps + {rest}; program_info h_tile_sweeps {pi['h_tile_sweeps']} h_untiled_groups "
          f"{pi['h_untiled_groups']} real_stream {pi['real_stream']}")
    assert len(sweeps) >= 2 and rest == 0
    if not pi["real_stream"]:
        assert (pi["h_tile_sweeps"], pi["h_untiled_groups"]) == (len(sweeps), 0), pi
    return len(sweeps)


# ---- A: the 16 | 17 boundary ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pairs():
    return {False: st.boundary_pair(leak=False), True: st.boundary_pair(leak=True)}


@pytest.mark.parametrize("call", ["single", "batch", "deflated", "spread", "spread_leak"])
def test_the_16_17_boundary(SV, pairs, call):
    """THE 16 | 17 BOUNDARY (COMPACT_MAX_QUBITS = 16: ``n_local > 16`` in run_sparse_gradient, run_grad_batch, run_vqd_batch,
    run_spread_batch).  One program — Y rotations on index bits 0 to 6, m = 128, K = 9 — on SV(16) and SV(17), the Hamiltonian at 17 the
    one at 16 term for term plus c Z on index bit 16: at 16 every call is on its compact path (a grad_* form for the single call), at 17
    on path 2 (launches 0 / 3 per vector pass + 1 per vector / 6 per row, reason 1, no grad_* form).  Each register meets its own
    checker (row 1), and the two registers each other: energies and costs differ by c (w_energy c for the spread call, whose omega is
    moved by c), spreads, overlaps and gradients by nothing, within the sum of the two bounds.  The deflated call holds J = 2: a complex
    vector — at 17 the 16-qubit one with zeros above — and an ansatz state.  "spread_leak": the pair with 0.3 X on index bit 9, which
    sends the spread call to path 2 at 16 as well (reason 3).  If COMPACT_MAX_QUBITS moves, ``stream_cases.boundary_pair`` moves with it."""
    lo, hi = pairs[call == "spread_leak"]
    c17 = st.BOUNDARY_C
    thetas = st.thetas(lo, 3, 1617)
    thetas[2] = thetas[0]
    ansatz = st.thetas(lo, 1, 1618)[0]
    vec = dc.random_vector(lo.n, 77)
    omegas = {16: np.array([0.4, -0.3, 0.4]), 17: np.array([0.4, -0.3, 0.4]) + c17}
    got, tols = {}, {}
    for case in (lo, hi):
        n, compact = case.n, case.n <= st.COMPACT_MAX_QUBITS
        what = f"{call} at {n}"
        with SV(n) as sv:
            case.load(sv)
            if call == "single":
                e, g = sv.energy_gradient(thetas[1])
                forms = sv.sparse_forms()
                print(f"{what}: sparse forms {sorted(forms)}; sector forms {sorted(sv.sector_forms())}")
                assert bool(forms & GRAD_FORMS) == compact
                out = (np.array([e]), g[None, :], np.array([e]), None)
                _plain_checker(case, thetas[1:2], out, [0], what)
                got[n], tols[n] = [out], case.tol_checker()
            elif call == "batch":
                out = _plain(sv, thetas)
                print(f"{what}: {out[4]}; sparse forms {sorted(sv.sparse_forms())}; sector forms {sorted(sv.sector_forms())}")
                if compact:
                    assert out[4]["path"] == 1 and out[4]["launches"] == 1 and out[4]["support"] == 128
                else:
                    _plain_path2(out[4])
                    assert not sv.sparse_forms() & GRAD_FORMS
                _plain_checker(case, thetas, out, [1], what)
                _plain_single(sv, case, thetas, out, [0, 2], what)
                got[n], tols[n] = [out], case.tol_checker()
            elif call == "deflated":
                held = Held()
                held.push_set(sv, [("vector", np.concatenate([vec, np.zeros(len(vec) * (2 ** (n - lo.n) - 1))]), 1.5), ("ansatz", ansatz, 2.5)])
                out = _deflated(sv, thetas, held)
                print(f"{what}: {out[4]}")
                if compact:
                    assert out[4]["path"] == 1 and out[4]["launches"] == 1 and out[4]["rows"] == 3 and out[4]["support"] == 128
                else:
                    _deflated_path2(out[4])
                    assert out[4]["launches"] == 3 * (2 + 2)
                _deflated_checker(case, held, thetas, out, [1], what)
                _deflated_single(sv, case, held, thetas, out, [0, 2], what)
                assert _same_bits(out[0][0], out[0][2]) and _same_bits(out[3][0].view(np.float64), out[3][2].view(np.float64))
                got[n], tols[n] = [out], dc.bound_checker(case.h1, case.C, held.vectors, held.betas)
            else:
                got[n], tols[n] = [], 0.0
                for omega in (None, omegas[n]):
                    out = _spread(sv, thetas, omega)
                    print(f"{what}: {out[4]}")
                    if compact and call == "spread":
                        assert out[4]["path"] == 1 and out[4]["launches"] == 1 and out[4]["why"] == 0 and out[4]["support"] == 128
                    else:
                        _spread_path2(out[4], why=3 if compact else 1)
                    _spread_checker(case, thetas, omega, out, [1], what)
                    _spread_single(sv, case, thetas, omega, out, [0, 2], what)
                    assert _same_bits(out[2][0], out[2][2]) and _same_bits(out[3][0], out[3][2])
                    got[n].append(out)
                    tols[n] = max(tols[n], sp.bound_checker(case, omega, WE, WS))
            if not compact:
                assert not sv.sparse_forms() & GRAD_FORMS
    tol = tols[16] + tols[17]
    for a, b in zip(got[16], got[17]):
        shift = WE * c17 if call.startswith("spread") else c17
        dcost, de, dg = _dev(b[0] - shift, a[0]), _dev(b[2] - c17, a[2]), _dev(b[1], a[1])
        dlast = 0.0 if a[3] is None else _dev(b[3], a[3])       # overlaps, spreads: the same on both registers
        print(f"{call}: 17 against 16: |dC - shift| {dcost:.3e} |dE - c| {de:.3e} max|dg| {dg:.3e} overlaps / spreads {dlast:.3e} bound {tol:.3e}")
        assert dcost <= tol and de <= tol and dg <= tol
        assert dlast <= (2e-12 if call == "deflated" else tol)     # two unit vectors: bound_overlap of each register


# ---- B: streaming rows at their own sizes --------------------------------------------------------------------------------------------------
def _three_rows(case, seed):
    thetas = st.thetas(case, 3, seed)
    thetas[2] = thetas[0]
    return thetas


def _checker_rows(n):
    """the checker's share of a test: two rows at 17 qubits, one from 19 on (seconds per row there)"""
    return [0, 1] if n < st.TILED_FROM else [0]


@pytest.mark.parametrize("real", [True, False])
@pytest.mark.parametrize("n", [17, 19, 20])
def test_streaming_rows_plain(SV, n, real):
    """ovqe_energy_gradient_batch row by row at 17 (k_apply_sum: below APPLY_MIN_TILES = 256 tiles of 2^TILE_BITS = 2^11), 19 (k_tile_apply
    from 2^19 amplitudes on, ident = 0 through two sweeps) and 20 qubits (the second grid-stride trip of k_dot and of every vector
    kernel: reduce_blocks caps at 2048 x 256 lanes, 2^19): path 2, launches 0; rows against the checker and against ovqe_energy_gradient;
    the repeated row and the repeated call give the same bits where the streaming kernels served (no sector form on the handle; a real
    program may run on the sector tables: then the same-handle bound)"""
    case = st.dense(n, real)
    thetas = _three_rows(case, 100 + n)
    what = f"plain dense({n}, {real})"
    with SV(n) as sv:
        case.load(sv)
        out = _plain(sv, thetas)
        again = _plain(sv, thetas)
        sector = sorted(sv.sector_forms())
        print(f"{what}: {out[4]}; trips {st.trips(n)}; tiled {st.tiled_by_default(n)}; sector forms {sector}")
        _apply_cover_of_the_handle(sv, case, what)
        _plain_path2(out[4])
        assert not sv.sparse_forms() & GRAD_FORMS
        if not sector:
            assert _all_same_bits(out[:2], again[:2]) and _same_bits(out[0][0], out[0][2]) and _same_bits(out[1][0], out[1][2])
        else:
            assert max(_dev(out[0], again[0]), _dev(out[1], again[1]), _dev(out[1][0], out[1][2])) <= case.tol_single()
        _plain_single(sv, case, thetas, out, range(3), what)
    _plain_checker(case, thetas, out, _checker_rows(n), what)


@pytest.mark.parametrize("real", [True, False])
@pytest.mark.parametrize("n", [17, 19, 20])
def test_streaming_rows_deflated(SV, n, real):
    """ovqe_deflated_gradient_batch on path 2 with J = 5 — a complex and a real random vector and three ansatz states: one full pass of
    DEFLATE_CHUNK = 4 and a remainder of one — at 17, 19 (lambda = H psi by k_tile_apply, ident = 0) and 20 qubits (the second trip of
    k_deflate_dots and k_deflate_axpy: 2048 workgroups of 256 on 2^20 amplitudes, 4 x 2048 partials).  Overlaps against the checker's
    np.vdot(phi_j, psi).  With no vector held: costs equal energies to the bit, and ovqe_energy_gradient_batch within the same-handle
    bound.  The repeated call and the repeated row give the same bits"""
    case = st.dense(n, real)
    thetas = _three_rows(case, 200 + n)
    what = f"deflated dense({n}, {real})"
    held = Held()
    with SV(n) as sv:
        case.load(sv)
        e0, g0 = sv.energy_gradient_batch(thetas)
        none = _deflated(sv, thetas, held)
        _deflated_path2(none[4])
        agree = _same_bits(none[2], e0)
        print(f"{what}: no vectors: energies equal energy_gradient_batch's to the bit: {agree}; max deviation {max(_dev(none[2], e0), _dev(none[1], g0)):.3e} "
              f"bound {case.tol_single():.3e}; sector forms {sorted(sv.sector_forms())}")
        assert none[4]["launches"] == 0 and _same_bits(none[0], none[2])
        assert _dev(none[2], e0) <= case.tol_single() and _dev(none[1], g0) <= case.tol_single()
        held.push_set(sv, st.vector_set(case, 5))
        out = _deflated(sv, thetas, held)
        again = _deflated(sv, thetas, held)
        print(f"{what}: {out[4]}; trips {st.trips(n)}; tiled {st.tiled_by_default(n)}")
        _apply_cover_of_the_handle(sv, case, what)
        _deflated_path2(out[4])
        assert out[4]["launches"] == 3 * 9
        assert all(_same_bits(np.ascontiguousarray(a).view(np.float64), np.ascontiguousarray(b).view(np.float64)) for a, b in zip(out[:4], again[:4]))
        assert _same_bits(out[0][0], out[0][2]) and _same_bits(out[1][0], out[1][2]) and _same_bits(out[3][0].view(np.float64), out[3][2].view(np.float64))
        _deflated_single(sv, case, held, thetas, out, [0, 1], what)
    _deflated_checker(case, held, thetas, out, _checker_rows(n), what)


@pytest.mark.parametrize("real", [True, False])
@pytest.mark.parametrize("n", [17, 19, 20])
def test_streaming_rows_spread(SV, n, real):
    """ovqe_spread_gradient_batch on path 2 (reason 1) in variance mode and with an omega per row, weights (0.3, 1.0), at 17, 19 (tau =
    (H - omega) sigma by k_tile_apply with ident = constant - omega through two sweeps: it enters in the first one only) and 20 qubits
    (the second trip of k_axpy_real with and without ``overwrite``, of k_scale, and of k_dot into 2048 partials for k_reduce).  One
    checker row per mode.  w = (1, 0) is the batched gradient within the same-handle bound.  The repeated call and the repeated row give
    the same bits"""
    case = st.dense(n, real)
    thetas = _three_rows(case, 300 + n)
    what = f"spread dense({n}, {real})"
    with SV(n) as sv:
        case.load(sv)
        e0, g0 = sv.energy_gradient_batch(thetas)
        outs = {}
        for omega in (None, np.array([0.4, -0.7, 0.4])):
            out = _spread(sv, thetas, omega)
            again = _spread(sv, thetas, omega)
            print(f"{what}: {out[4]}; trips {st.trips(n)}; tiled {st.tiled_by_default(n)}")
            _spread_path2(out[4])
            assert _all_same_bits(out, again) and all(_same_bits(a[0], a[2]) for a in out[:4])
            _spread_single(sv, case, thetas, omega, out, [1, 2], what)
            outs[omega is None] = (omega, out)
            c, g, e, s, _ = _spread(sv, thetas, omega, 1.0, 0.0)
            tol = sp.bound_single(case, omega, 1.0, 0.0)
            print(f"   {what}: w = (1, 0) against energy_gradient_batch: {max(_dev(c, e0), _dev(e, e0), _dev(g, g0)):.3e} bound {tol:.3e}")
            assert max(_dev(c, e0), _dev(e, e0), _dev(g, g0)) <= tol
        _apply_cover_of_the_handle(sv, case, what)
    for omega, out in outs.values():
        _spread_checker(case, thetas, omega, out, [0] if omega is None else [1], what)


# ---- C: both forms of H psi under every streaming row ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, real", [(13, False), (14, True)])
def test_both_forms_of_h_psi(SV, n, real):
    """K_TILE_APPLY INSIDE THE NEW CALLS, on registers small enough for the checker on every row: "force_path" 2 and "apply_min_tiles" 1
    (k_tile_apply, tiles of 2^TILE_BITS = 2^11: four and eight of them), then 2^30 (the gather kernel k_apply_sum), then 1 again, on one
    handle — both orders.  Precondition asserted on the handle: the cover of the Hamiltonian has at least two sweeps and no untiled
    rest, so an identity part added in every sweep instead of the first would enter twice.  The spread call runs with omega_b =
    constant - ||H||_1 (1, 0.8, 1): ident = constant - omega of order ||H||_1, far above every bound in lambda — and in variance mode;
    the deflated (J = 5) and the plain rows pass ident = 0 through the same sweeps.  The three calls agree across the two forms within
    the same-handle bounds, meet the checker under both, and the first and the third pass give the same bits.  The real program runs
    with "real_stream" 0: the plain rows stream too, and ovqe_program_info describes the cover of the complex register"""
    case = st.dense(n, real)
    thetas = _three_rows(case, 400 + n)
    what = f"dense({n}, {real})"
    h1 = float(np.abs(case.h[2]).sum())
    omega_far = case.h[3] - h1 * np.array([1.0, 0.8, 1.0])
    assert np.abs(case.h[3] - omega_far).min() >= 0.8 * h1 - 1e-12 and 0.8 * h1 >= 1e6 * sp.bound_checker(case, omega_far, WE, WS)
    held = Held()
    runs = []
    with SV(n) as sv:
        sv.set_option("force_path", 2)
        if real:
            sv.set_option("real_stream", 0)
        case.load(sv)
        held.push_set(sv, st.vector_set(case, 5))
        for tiles in (1, st.NO_TILES, 1):
            sv.set_option("apply_min_tiles", tiles)
            form = "k_tile_apply" if tiles == 1 else "k_apply_sum"
            run = {"plain": _plain(sv, thetas), "deflated": _deflated(sv, thetas, held), "variance": _spread(sv, thetas, None),
                   "omega": _spread(sv, thetas, omega_far)}
            if not runs:
                nsweeps = _apply_cover_of_the_handle(sv, case, what)
                assert sv.program_info()["real_stream"] == 0 and nsweeps >= 2
            _plain_path2(run["plain"][4])
            _deflated_path2(run["deflated"][4])
            _spread_path2(run["variance"][4])
            _spread_path2(run["omega"][4])
            assert not sv.sector_forms() and not sv.sparse_forms() & GRAD_FORMS
            _plain_checker(case, thetas, run["plain"], [0, 1], f"{what} {form}")
            _deflated_checker(case, held, thetas, run["deflated"], [0, 1], f"{what} {form}")
            _spread_checker(case, thetas, None, run["variance"], [0, 1], f"{what} {form}")
            _spread_checker(case, thetas, omega_far, run["omega"], [0, 1], f"{what} {form}")
            runs.append(run)
    tols = {"plain": case.tol_single(), "deflated": dc.bound_single(case.h1, case.C, held.vectors, held.betas),
            "variance": sp.bound_single(case, None, WE, WS), "omega": sp.bound_single(case, omega_far, WE, WS)}
    for name, tol in tols.items():
        tiled, gather, tiled_again = (r[name] for r in runs)
        last = 2 if name == "plain" else 4
        d = max(_dev(a, b) for a, b in zip(tiled[:last], gather[:last]))
        print(f"{what} {name}: k_tile_apply against k_apply_sum: {d:.3e} bound {tol:.3e}")
        assert d <= tol
        assert all(_same_bits(np.ascontiguousarray(a).view(np.float64), np.ascontiguousarray(b).view(np.float64)) for a, b in zip(tiled[:last], tiled_again[:last]))


def test_the_gather_form_on_two_trips(SV):
    """THE SECOND TRIP OF k_apply_sum: at 20 qubits the default is the tiled form, so one row runs with "apply_min_tiles" 2^30 — 2048
    workgroups of 256 on 2^20 amplitudes, every lane twice — for the plain, the deflated (J = 1: a remainder pass alone) and the spread
    call, against the tiled rows of the same handle within the same-handle bounds.  No checker row: the tiled rows meet it in
    test_streaming_rows_*"""
    case = st.dense(20, False)
    assert st.trips(20) == 2 and st.tiled_by_default(20)
    thetas = st.thetas(case, 1, 520)
    omega = np.array([-0.7])
    held = Held()
    with SV(20) as sv:
        case.load(sv)
        held.push_set(sv, st.vector_set(case, 1))
        runs = []
        for tiles in (st.APPLY_MIN_TILES, st.NO_TILES):
            sv.set_option("apply_min_tiles", tiles)
            runs.append((_plain(sv, thetas), _deflated(sv, thetas, held), _spread(sv, thetas, None), _spread(sv, thetas, omega)))
        _apply_cover_of_the_handle(sv, case, "dense(20, False)")
        _deflated_path2(runs[1][1][4])
        assert runs[1][1][4]["launches"] == 3
    tols = (case.tol_single(), dc.bound_single(case.h1, case.C, held.vectors, held.betas), sp.bound_single(case, None, WE, WS),
            sp.bound_single(case, omega, WE, WS))
    for k, (name, tol) in enumerate(zip(("plain", "deflated", "variance", "omega"), tols)):
        last = 2 if name == "plain" else 4
        d = max(_dev(a, b) for a, b in zip(runs[0][k][:last], runs[1][k][:last]))
        print(f"dense(20, False) {name}: k_apply_sum on two trips against k_tile_apply: {d:.3e} bound {tol:.3e}")
        assert d <= tol


# ---- D: the vector count ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", [1, 2])
def test_the_vector_count(SV, path):
    """THE VECTOR COUNT OF DEFLATION (DEFLATE_MAX = 32, DEFLATE_CHUNK = 4) on ``gradbatch_cases.per_rotation(9)`` (7 qubits, the support is
    the register), B = 3, on path 1 and under "force_path" 2, with the nested sets of ``stream_cases.nested_set``: J = 1 (path 2: a
    remainder pass alone), 4 (exactly one pass), 5 (a pass and a remainder of one), 32 (eight full passes, slots 0 to 31 of the 64-slot
    d_result; path 1: thirty complex vectors, a real one and the real ansatz state are 2 x 30 + 1 + 1 = 62 real rows of D — derived from
    the vectors read back from the handle).  Costs, gradients and every overlap, both parts, against the checker on all rows.  Then
    ovqe_deflation_truncate(4) on the same handle: the J = 4 answers again within the same-handle bound"""
    case = gc.per_rotation(9)
    thetas = st.thetas(case, 3, 32)
    nested = st.nested_set(case)
    held = Held()
    kept = None
    with SV(case.n) as sv:
        sv.set_option("force_path", 0 if path == 1 else 2)
        case.load(sv)
        for J in (1, 4, 5, 32):
            held.push_set(sv, nested[len(held.vectors):J])
            out = _deflated(sv, thetas, held)
            info = out[4]
            rows = st.real_rows(held.vectors)
            print(f"path {path} J = {J}: {info}; real rows derived {rows}")
            assert rows == J + sum(1 for k in range(J) if k not in (1, 2))
            if path == 1:
                assert info["path"] == 1 and info["launches"] == 1 and info["rows"] == rows and info["support"] == 128 and info["gather_launches"] == 1
                assert J != 32 or info["rows"] == 62
            else:
                _deflated_path2(info)
                assert info["launches"] == 3 * {1: 3, 4: 6, 5: 9, 32: 48}[J]
            _deflated_checker(case, held, thetas, out, range(3), f"path {path} J {J}")
            if J == 4:
                kept = out
        assert sv.deflation_count() == st.DEFLATE_MAX
        held.truncate(sv, 4)
        out = _deflated(sv, thetas, held)
        assert out[4]["path"] == path and (path == 2 or (out[4]["rows"] == 6 and out[4]["gather_launches"] == 1))
        tol = dc.bound_single(case.h1, case.C, held.vectors, held.betas)
        d = max(_dev(a, b) for a, b in zip(out[:3], kept[:3]))
        print(f"path {path}: J = 4 after truncation against J = 4 before: {d:.3e} bound {tol:.3e}; overlaps {_dev(out[3], kept[3]):.2e}")
        assert d <= tol and _dev(out[3], kept[3]) <= 1e-12
        _deflated_checker(case, held, thetas, out, [1], f"path {path} J 4 again")


# ---- E: one handle, every call ------------------------------------------------------------------------------------------------------------
def test_one_handle_every_call(SV):
    """SHARED SCRATCH ACROSS CALLS ON ONE HANDLE (d_partials, d_result, scratch[0]) on ``dense(20, False)`` — 2^20 amplitudes: reduce_blocks
    = 2048, DEFLATE_CHUNK x 2048 partials for the deflated rows, ADJ_MAX_ROT x 2048 for every backward walk, 2048 for vec_dot; the spread
    call's work vectors are its own.  In order: ovqe_energy_gradient, the deflated call (J = 5), the spread call (variance, then omega
    given), ovqe_energy_gradient_batch, ovqe_energy, ovqe_energy_gradient — and the whole sequence again: every result of the second round
    equals the first to the bit, the single energy and gradient after the batched calls equal those before them to the bit (what the
    header promises in the place of a specified state buffer), and the energies of all calls agree within the same-handle bound.  No
    checker row.

    Then a fresh 17-qubit handle serves a J = 32 deflated call (eight passes over 512 workgroups; all 32 overlaps against np.vdot with the
    state the handle prepares) on ``dense(17, False)``, and after it ``boundary_pair``'s 17-qubit case with the 32 vectors still held:
    the single, the batched, the spread and the deflated call against the checker — nothing sized for one call is assumed by the next"""
    case = st.dense(20, False)
    thetas = st.thetas(case, 2, 620)
    omega = np.array([0.4, -0.7])
    held = Held()

    def sequence(sv):
        e0, g0 = sv.energy_gradient(thetas[0])
        d = _deflated(sv, thetas, held)
        v = _spread(sv, thetas, None)
        w = _spread(sv, thetas, omega)
        p = _plain(sv, thetas)
        e1 = sv.energy(thetas[0])
        e2, g2 = sv.energy_gradient(thetas[0])
        assert np.float64(e0).view(np.int64) == np.float64(e2).view(np.int64) and _same_bits(g0, g2)
        _deflated_path2(d[4])
        _spread_path2(v[4])
        _spread_path2(w[4])
        _plain_path2(p[4])
        return [np.array([e0]), g0, d[0], d[1], d[2], d[3].view(np.float64), v[0], v[1], v[2], v[3], w[0], w[1], w[2], w[3], p[0], p[1], np.array([e1])]

    with SV(20) as sv:
        case.load(sv)
        held.push_set(sv, st.vector_set(case, 5))
        first = sequence(sv)
        second = sequence(sv)
    assert all(_same_bits(a, b) for a, b in zip(first, second))
    tol = case.tol_single()
    e0, energies = first[0][0], [first[4][0], first[8][0], first[12][0], first[14][0], first[16][0]]
    print(f"dense(20, False): the energy of row 0 by six calls: spread {max(abs(e - e0) for e in energies):.3e} bound {tol:.3e}")
    assert all(abs(e - e0) <= tol for e in energies) and _dev(first[15][0], first[1]) <= tol

    big, (_, hi) = st.dense(17, False), st.boundary_pair(leak=False)
    held = Held()
    theta_big = st.thetas(big, 1, 621)
    thetas = st.thetas(hi, 2, 622)
    with SV(17) as sv:
        big.load(sv)
        rng = np.random.default_rng(623)
        for j in range(st.DEFLATE_MAX):
            held.push_set(sv, [("vector", dc.random_vector(17, 700 + j, real=j % 5 == 4), float(rng.uniform(0.25, 1.0)))])
        out = _deflated(sv, theta_big, held)
        _deflated_path2(out[4])
        assert out[4]["launches"] == 48 and out[4]["J"] == 32
        sv.prepare_state(theta_big[0])
        psi = sv.get_state()
        want = np.array([np.vdot(v, psi) for v in held.vectors])
        print(f"dense(17, False) J = 32: max overlap deviation {np.abs(out[3][0] - want).max():.2e} bound 1e-12; min |o| {np.abs(want).min():.2e}")
        assert np.abs(out[3][0] - want).max() <= 1e-12
        pen = sum(b * abs(o) ** 2 for b, o in zip(held.betas, want))
        assert abs(out[0][0] - out[2][0] - pen) <= dc.bound_single(big.h1, big.C, held.vectors, held.betas)
        hi.load(sv)
        assert sv.deflation_count() == 32
        e, g = sv.energy_gradient(thetas[0])
        p = _plain(sv, thetas)
        v = _spread(sv, thetas, None)
        d = _deflated(sv, thetas, held)
        _plain_path2(p[4])
        _spread_path2(v[4])
        _deflated_path2(d[4])
        assert abs(e - p[0][0]) <= hi.tol_single() and _dev(g, p[1][0]) <= hi.tol_single()
    _plain_checker(hi, thetas, p, [0], "boundary case at 17 after J = 32")
    _spread_checker(hi, thetas, None, v, [1], "boundary case at 17 after J = 32")
    _deflated_checker(hi, held, thetas, d, [0], "boundary case at 17 after J = 32")
