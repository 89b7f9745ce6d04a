"""tests/sector_cases.py on the CPU: the support-only gradient reference against the dense-register adjoint pass and against central
differences of the C oracle, and the constructions of the counted-magnitude Hamiltonian."""
import numpy as np
import pytest

from oracle import cref, masks
from tests import sector_cases as sc


@pytest.fixture(scope="module", autouse=True)
def _oracle_built():
    cref.build()


def _dense_gradient(case, theta):
    return masks.ucc_energy_gradient(case.n, case.hf, case.rx, case.rz, case.rc, case.pidx, theta, case.hx, case.hz, case.hc,
                                     case.ham.constant_coeff)


@pytest.mark.parametrize("make", [lambda: sc.molecule(7, 2), lambda: sc.molecule(7, 2, singles_only=True), lambda: sc.counted_case(150)],
                         ids=["uccsd(7,2)", "singles(7,2)", "counted(150)"])
def test_support_gradient_equals_the_dense_register_adjoint_pass(make):
    """same mathematics on the support as on the register, both complex128: 1e-12 max(1, |H|_1) on the energy and on every component
    (a thousand rotations of unit-modulus arithmetic: rounding of a few 1e-14), at generic angles and at zero"""
    case = make()
    for theta in case.thetas(2, seed=1):
        e_dense, g_dense = _dense_gradient(case, theta)
        e_sup, g_sup = case.gradient(theta)
        print(f"{case.name}: |dE| = {abs(e_sup - e_dense):.2e}, max |dg| = {np.abs(g_sup - g_dense).max():.2e}, bound {1e-12 * case.bound:.2e}")
        assert abs(e_sup - e_dense) < 1e-12 * case.bound and abs(e_sup - case.energy(theta)) < 1e-12 * case.bound
        assert np.abs(g_sup - g_dense).max() < 1e-12 * case.bound
        assert np.abs(g_dense).max() > 1e-3 or not np.any(theta)


@pytest.mark.parametrize("make", [lambda: sc.molecule(7, 2), lambda: sc.counted_case(150)], ids=["uccsd(7,2)", "counted(150)"])
def test_support_gradient_against_central_differences_of_the_c_oracle(make):
    """a few components against (E(theta + h e_k) - E(theta - h e_k)) / 2h of the C oracle, h = 1e-5, within 1e-6 max(1, |H|_1) — the
    bound tests/test_gpu_sector.py::test_sector_adjoint_gradient uses"""
    case = make()
    theta = case.thetas(2, seed=2)[0]
    _, grad = case.gradient(theta)
    rng = np.random.default_rng(5)
    h = 1e-5
    for k in rng.choice(case.K, 4, replace=False):
        tp, tm = theta.copy(), theta.copy()
        tp[k] += h
        tm[k] -= h
        fd = (case.energy(tp) - case.energy(tm)) / (2 * h)
        print(f"{case.name}: component {k}: reference {grad[k]:+.12f}, differences {fd:+.12f}")
        assert abs(fd - grad[k]) < 1e-6 * case.bound, k


def test_counted_program_has_the_stated_support():
    """13-bit strings without (bit 11 and bit 12), the other three index bits as in |hf>: 6144 amplitudes in one 13-bit tile, and every
    mask inside the 13 bits connects two of them"""
    case = sc.counted_case(150)
    low = np.array([s for s in range(1 << sc.COUNTED_BITS) if (s >> 11) & 3 != 3], np.uint64)
    assert len(low) == sc.COUNTED_SUPPORT
    assert np.array_equal(case.support, np.uint64(case.hf) | low)
    assert all(sc.connected(case.support, int(x)) for x in sc.counted_masks()[::97])
    assert len(sc.counted_masks()) == 8100


@pytest.mark.parametrize("target", sorted(sc.COUNTED_GROUPS))
def test_counted_hamiltonian_has_the_stated_number_of_connected_groups(target):
    """per target dictionary size: that many X groups, pairwise distinct masks of weight >= 3 inside the 13 bits, each connecting two
    members of the support, pairwise distinct magnitudes none of which is the diagonal term's; real symmetric"""
    groups = sc.COUNTED_GROUPS[target]
    case = sc.counted_case(groups)
    assert groups + sc.COUNTED_DICT_EXTRA == target
    nz = case.hx != 0
    xs = case.hx[nz]
    assert len(xs) == groups == len(set(xs.tolist())) == len(case.kept) and np.count_nonzero(~nz) == 1
    assert all(bin(int(x)).count("1") >= 3 and int(x) < (1 << sc.COUNTED_BITS) for x in xs)
    assert all(sc.connected(case.support, int(x)) for x in xs)
    assert np.all(case.hz[nz] == 0)                                            # X only: every element of a group is c_x
    assert len(set(np.abs(case.hc).tolist())) == groups + 1
    # real symmetric: real coefficients on strings without Y, and <u|H v> = <v|H u> on the support
    assert case.hc.dtype == np.float64 and np.all((case.hx & case.hz) == 0)
    rng = np.random.default_rng(target)
    u, v = rng.normal(size=(2, len(case.support)))
    hu, hv = (sc.apply_on_support(case.support, w.astype(np.complex128), case.hx, case.hz, case.hc) for w in (u, v))
    assert np.abs(hu.imag).max() == 0.0 and abs(np.dot(v, hu.real) - np.dot(u, hv.real)) < 1e-10 * case.bound


def test_counted_hamiltonian_energy_from_the_mask_oracle_equals_the_c_oracle():
    """<psi|H|psi> with ``oracle.masks.apply_pauli_sum`` on the C oracle's state, the C oracle's own energy and the support-only
    product of sector_cases agree to 1e-12 max(1, |H|_1)"""
    case = sc.counted_case(150)
    for theta in case.thetas(2, seed=3):
        e_c, psi = case.oracle(theta)
        sigma = masks.apply_pauli_sum(psi, case.hx, case.hz, case.hc)
        e_masks = float(np.vdot(psi, sigma).real) + case.ham.constant_coeff
        idx = case.support.astype(np.int64)
        on_support = sc.apply_on_support(case.support, psi[idx], case.hx, case.hz, case.hc)
        assert abs(e_masks - e_c) < 1e-12 * case.bound
        assert np.abs(on_support - sigma[idx]).max() < 1e-12 * case.bound
