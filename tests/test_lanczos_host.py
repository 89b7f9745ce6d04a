"""The Lanczos recurrence of the ground-state solvers (openvqe_amd/csrc/sv_lanczos_host.hpp: lanczos_lowest over a Space, tridiag_lowest)
compiled with g++ alone under ASan + UBSan: tests/cpu/lanczos_check.cpp runs it on dense symmetric matrices — two-pass, one-pass from
kept vectors, with the budget running out, under a mask (the sector's reachable block), at breakdown, on one dimension and with a failing
operator.  Energies against numpy.linalg.eigvalsh to 1e-9 scale and true residuals below 1e-6 scale, scale = max(1, |A|_inf): the bounds
of tests/test_gpu_kernels.py::test_ground_state_lanczos on the device."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL, MAX_ITER = "1e-11", "3000"


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    """run(matrix, start, mode, mask=None) -> (fields of the program's output line, Ritz vector, alpha, beta)"""
    tmp = tmp_path_factory.mktemp("lanczos")
    src = os.path.join(ROOT, "tests", "cpu", "lanczos_check.cpp")
    exe = str(tmp / "lanczos_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-o", exe, src])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    count = [0]

    def run(a, start, mode, mask=None):
        count[0] += 1
        n = a.shape[0]
        inp, out = str(tmp / f"in{count[0]}.bin"), str(tmp / f"out{count[0]}.bin")
        with open(inp, "wb") as f:
            np.array([n, 0 if mask is None else 1], dtype=np.int64).tofile(f)
            np.ascontiguousarray(a, dtype=np.float64).tofile(f)
            if mask is not None:
                np.asarray(mask, dtype=np.float64).tofile(f)
            np.asarray(start, dtype=np.float64).tofile(f)
        r = subprocess.run([exe, inp, mode, TOL, MAX_ITER, out], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
        f = dict(kv.split("=") for kv in r.stdout.split())
        res = {"rc": int(f["rc"]), "lam": float(f["lam"]), "residual": float(f["residual"]), "m": int(f["m"]), "hash": f["hash"],
               "tlam": float(f["tlam"]), "snorm2m1": float(f["snorm2m1"]), "after_failure": int(f["after_failure"])}
        if res["rc"]:
            return res, None, None, None
        v = np.fromfile(out, dtype=np.float64)
        m = res["m"]
        assert v.size == n + 2 * m - 1
        return res, v[:n], v[n:n + m], v[n + m:]

    return run


def _scale(a):
    return max(1.0, np.abs(a).sum(axis=1).max())


def _assert_lowest(res, a, ref=None):
    scale = _scale(a)
    ref = np.linalg.eigvalsh(a)[0] if ref is None else ref
    print(f"lam - ref = {res['lam'] - ref:.3e}, residual = {res['residual']:.3e}, m = {res['m']}, scale = {scale:.3g}")
    assert res["rc"] == 0
    assert abs(res["lam"] - ref) < 1e-9 * scale
    assert res["residual"] < 1e-6 * scale


def _random_symmetric(rng, n):
    a = rng.uniform(-1.0, 1.0, (n, n))
    return 0.5 * (a + a.T)


def _path_laplacian(n):
    """the second-difference matrix of a path, fixed ends: eigenvalues 2 - 2 cos(k pi / (n + 1))"""
    return 2.0 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1)


def test_path_graph_laplacian_runs_every_step_and_its_tridiagonal_matrix(check):
    """Case 1: gap 7e-3 on 64 dimensions, all 64 steps.  Case 8: tridiag_lowest alone on its (alpha, beta)."""
    a = _path_laplacian(64)
    res, _, alpha, beta = check(a, np.random.default_rng(1).standard_normal(64), "two")
    _assert_lowest(res, a)
    assert res["m"] == 64
    t = np.diag(alpha) + np.diag(beta, 1) + np.diag(beta, -1)
    assert abs(res["tlam"] - np.linalg.eigvalsh(t)[0]) < 1e-12 * _scale(a)
    assert abs(res["snorm2m1"]) < 1e-12


def test_random_symmetric_matrix(check):
    """Case 2: 48 x 48, converges near step 40."""
    rng = np.random.default_rng(2)
    a = _random_symmetric(rng, 48)
    res, _, _, _ = check(a, rng.standard_normal(48), "two")
    _assert_lowest(res, a)
    assert res["m"] < 48


def test_one_pass_from_kept_vectors_is_the_two_pass_result(check):
    """Case 3: 200 x 200, converges well before step 200; with every vector kept, and with a budget of 10 vectors that runs out."""
    rng = np.random.default_rng(3)
    a = _random_symmetric(rng, 200) + np.diag(0.1 * np.arange(200))
    start = rng.standard_normal(200)
    two, y2, _, _ = check(a, start, "two")
    _assert_lowest(two, a)
    assert two["m"] < 200
    for mode in ("keep", "keep10"):
        one, y1, _, _ = check(a, start, mode)
        _assert_lowest(one, a)
        assert (one["m"], one["hash"]) == (two["m"], two["hash"])
        assert np.abs(y1 - y2).max() < 1e-12
        assert mode == "keep" or np.array_equal(y1, y2)   # budget spent: the same pass 2


def test_breakdown_on_three_levels(check):
    """Case 4: three distinct eigenvalues, the Krylov space has three dimensions."""
    a = np.diag(np.repeat([-1.5, 0.25, 2.0], 10))
    res, _, _, _ = check(a, np.random.default_rng(4).standard_normal(30), "two")
    _assert_lowest(res, a)
    assert res["m"] == 3


def test_mask_keeps_the_recurrence_inside_its_block(check):
    """Case 5: two blocks of 24, the unmasked one lower by 5: the lowest eigenvalue of the FIRST block, nothing outside the mask."""
    rng = np.random.default_rng(5)
    a = np.zeros((48, 48))
    a[:24, :24] = _random_symmetric(rng, 24)
    a[24:, 24:] = _random_symmetric(rng, 24) - 5.0 * np.eye(24)
    mask = np.r_[np.ones(24), np.zeros(24)]
    res, y, _, _ = check(a, rng.standard_normal(48), "two", mask)
    _assert_lowest(res, a, ref=np.linalg.eigvalsh(a[:24, :24])[0])
    assert np.all(y[24:] == 0.0)
    assert res["m"] <= 24


def test_one_dimension(check):
    """Case 6."""
    a = np.array([[-0.75]])
    res, y, _, _ = check(a, np.array([2.0]), "two")
    _assert_lowest(res, a)
    assert res["m"] == 1 and res["lam"] == -0.75 and abs(y[0]) == 1.0


def test_a_failing_operator_ends_the_solve_with_its_code(check):
    """Case 7: the third apply() returns 7; so does lanczos_lowest, and no vector operation follows."""
    rng = np.random.default_rng(7)
    res, _, _, _ = check(_random_symmetric(rng, 48), rng.standard_normal(48), "fail3")
    assert res["rc"] == 7 and res["after_failure"] == 0
