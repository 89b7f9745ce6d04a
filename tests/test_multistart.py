"""CPU tests of the lock-step multi-start optimiser (openvqe_amd/common_files/multistart.py) on analytic batched functions, and of
``replicas.energy_gradient_batch`` under gloo at world size 2 with a stub backend."""
import multiprocessing as mp
import os
import socket

import numpy as np
import pytest

from openvqe_amd.common_files import multistart


class Counted:
    """a batched function that records the rows of every call"""

    def __init__(self, fun_grad):
        self.fun_grad, self.calls = fun_grad, []

    def __call__(self, X):
        X = np.asarray(X, float)
        self.calls.append(X.copy())
        out = [self.fun_grad(x) for x in X]
        return np.array([f for f, _ in out]), np.array([g for _, g in out]).reshape(X.shape)


def double_well(x):
    """separable: sum_k (x_k^2 - 1)^2 + 0.3 x_0 — minima near x_k = +-1, the lowest with x_0 near -1"""
    f = float(np.sum((x * x - 1.0) ** 2) + 0.3 * x[0])
    g = 4.0 * x * (x * x - 1.0)
    g[0] += 0.3
    return f, g


def rosenbrock(x):
    f = float(np.sum(100.0 * (x[1:] - x[:-1] ** 2) ** 2 + (1.0 - x[:-1]) ** 2))
    g = np.zeros_like(x)
    g[:-1] = -400.0 * x[:-1] * (x[1:] - x[:-1] ** 2) - 2.0 * (1.0 - x[:-1])
    g[1:] += 200.0 * (x[1:] - x[:-1] ** 2)
    return f, g


def test_starts_on_either_side_reach_different_minima_and_the_best_is_returned():
    tol = 1e-9
    X0 = np.array([[0.6, 0.5], [-0.6, 0.5], [0.7, -0.4], [-0.5, -0.6]])
    fun = Counted(double_well)
    res = multistart.minimize(fun, X0, tol=tol, maxiter=200)
    print(res.message, res.nit, res.ncalls, res.rows, res.F, res.X)
    assert res.converged.all() and res.success
    assert np.all(np.sign(res.X) == np.sign(X0))            # every start stays in its own well
    assert np.allclose(np.abs(res.X[:, 1]), 1.0, atol=1e-8)
    right, left = res.F[0], res.F[1]
    assert left < right - 0.5 and res.fun == res.F.min() and res.best in (1, 3) and res.x[0] < 0
    assert np.array_equal(res.x, res.X[res.best]) and np.array_equal(res.jac, res.G[res.best]) and res.nit == res.iterations[res.best]
    # converged <=> gradient within the tolerance, per start
    assert np.array_equal(res.converged, np.abs(res.G).max(axis=1) <= tol)
    # the accepted energies never rise, and they are the best start's
    assert np.all(np.diff(res.energies) <= 0.0) and res.energies[0] == double_well(X0[res.best])[0] and res.energies[-1] == res.fun
    assert len(res.energies) == res.nit + 1
    # every call carries the active starts only
    assert res.ncalls == len(fun.calls) and res.rows == sum(len(c) for c in fun.calls)
    assert len(fun.calls[0]) == 4 and len(fun.calls[-1]) < 4 and res.rows < res.ncalls * 4
    assert all(len(a) >= len(b) for a, b in zip(fun.calls[1:], fun.calls[2:]))


def test_per_start_energies_never_rise_and_a_stalled_start_is_not_converged():
    """every start's accepted energies through a wrapper that follows the accepted points; maxiter = 3 leaves starts unconverged"""
    X0 = np.random.default_rng(3).uniform(-1.5, 1.5, (5, 4))
    res = multistart.minimize(Counted(rosenbrock), X0, tol=1e-8, maxiter=3)
    assert not res.converged.any() and np.all(res.iterations == 3) and not res.success and res.status == 1
    assert np.array_equal(res.converged, np.abs(res.G).max(axis=1) <= 1e-8)
    assert np.all(res.F <= [rosenbrock(x)[0] for x in X0])
    full = multistart.minimize(Counted(rosenbrock), X0, tol=1e-8, maxiter=2000)
    # (the four-dimensional Rosenbrock function has a second, local minimum near x_0 = -0.78: a start may end there)
    assert full.converged.all() and np.abs(full.G).max() <= 1e-8 and np.all(full.F <= res.F)
    assert np.allclose(full.x, 1.0, atol=1e-6) and full.fun < 1e-12
    for b in range(5):   # a start alone accepts the same energies as in company: its whole run is the same
        alone = multistart.minimize(Counted(rosenbrock), X0[b:b + 1], tol=1e-8, maxiter=2000)
        assert np.all(np.diff(alone.energies) <= 0.0)
        assert alone.fun == full.F[b] and np.array_equal(alone.x, full.X[b]) and alone.nit == full.iterations[b]


def test_one_row_is_row_0_of_a_run_on_copies_and_the_result_is_deterministic():
    x0 = np.array([-1.2, 1.0, 0.7])
    one = multistart.minimize(Counted(rosenbrock), x0[None, :], tol=1e-8, maxiter=2000)
    many = multistart.minimize(Counted(rosenbrock), np.tile(x0, (3, 1)), tol=1e-8, maxiter=2000)
    again = multistart.minimize(Counted(rosenbrock), np.tile(x0, (3, 1)), tol=1e-8, maxiter=2000)
    assert one.success and np.allclose(one.x, 1.0, atol=1e-6)
    assert np.array_equal(one.x, many.X[0]) and one.fun == many.F[0] and one.energies == many.energies and one.ncalls == many.ncalls
    assert np.array_equal(many.X[0], many.X[1]) and np.array_equal(many.X[0], many.X[2]) and many.best == 0 and many.rows == 3 * one.rows
    for key in ("x", "fun", "jac", "nit", "ncalls", "rows", "energies", "X", "F", "G", "converged", "iterations", "message"):
        assert np.array_equal(np.asarray(many[key]), np.asarray(again[key])), key
    flat = multistart.minimize(Counted(rosenbrock), x0, tol=1e-8, maxiter=2000)   # a vector is one start
    assert np.array_equal(flat.x, one.x)
    with pytest.raises(ValueError):
        multistart.minimize(Counted(rosenbrock), np.zeros((0, 3)))


def test_a_converged_start_costs_one_row():
    res = multistart.minimize(Counted(lambda x: (float(x @ x), 2.0 * x)), np.array([[0.0, 0.0], [3.0, -4.0]]), tol=1e-10)
    assert res.converged.all() and res.iterations[0] == 0 and res.best == 0 and res.rows == 2 + (res.ncalls - 1)


# ---- replicas.energy_gradient_batch under gloo -----------------------------------------------------------------------------------------
class StubBackend:
    """rows in, a recognisable energy and gradient per row out; records the rows it was given"""

    def __init__(self):
        self.seen = []

    def energy_gradient_batch(self, thetas):
        thetas = np.asarray(thetas, float)
        self.seen.append(thetas.copy())
        return thetas.sum(axis=1) + 0.5, 2.0 * thetas + np.arange(thetas.shape[1])[None, :]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank(rank, world, port, out):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from openvqe_amd import replicas
        assert replicas.active(4)
        results = {}
        for B in (0, 1, 3):
            sv = StubBackend()
            thetas = np.arange(B * 5, dtype=float).reshape(B, 5) / 7.0
            e, g = replicas.energy_gradient_batch(sv, thetas)
            results[B] = (e, g, [len(s) for s in sv.seen])
        out.put((rank, results))
    finally:
        dist.destroy_process_group()


def test_replicas_energy_gradient_batch_under_gloo():
    """world size 2: every rank receives all rows in order for B = 0, 1, 3, and evaluates only its share"""
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank, args=(r, 2, port, out)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(out.get(timeout=300) for _ in range(2))
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    shares = {0: ([], []), 1: ([1], []), 3: ([2], [1])}
    for rank in (0, 1):
        for B in (0, 1, 3):
            e, g, seen = got[rank][B]
            thetas = np.arange(B * 5, dtype=float).reshape(B, 5) / 7.0
            assert e.shape == (B,) and g.shape == (B, 5)
            assert np.array_equal(e, thetas.sum(axis=1) + 0.5) and np.array_equal(g, 2.0 * thetas + np.arange(5)[None, :])
            assert seen == shares[B][rank]
