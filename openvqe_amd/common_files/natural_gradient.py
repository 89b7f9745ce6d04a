"""Natural-gradient descent on the energy of a parameterised state — the counterpart of the gradient-descent optimiser with
``natural_gradient=True`` of the qat-variational package the reference's requirements pin.

With the Fubini-Study metric g(theta) of the ansatz state (``Statevector.metric_tensor``) the step

    (g + lambda I) delta = -grad E / 2

is one step of imaginary-time evolution projected on the ansatz manifold (McLachlan's variational principle): unlike the plain
gradient it does not depend on how the parameters are scaled or duplicated, which is what the redundant parameterisations of UCC and
ADAPT ansaetze need.  lambda is RELATIVE to the mean diagonal entry trace(g) / K, so that directions the state does not depend on
(zero rows of g) stay bounded.  The step length along delta comes from a backtracking (Armijo) line search on the energy that starts
from twice the length accepted before: the energy never rises.
"""
import numpy as np
import scipy.linalg
import scipy.optimize


def natural_step(metric, grad, damping=1e-6):
    """delta of (g + lambda I) delta = -grad / 2 with lambda = damping * trace(g) / K (damping itself when g vanishes)"""
    metric = np.asarray(metric, np.float64)
    grad = np.asarray(grad, np.float64)
    K = grad.shape[0]
    mean = float(np.trace(metric)) / max(K, 1)
    lam = damping * (mean if mean > 0.0 else 1.0)
    a = 0.5 * (metric + metric.T) + lam * np.eye(K)
    try:
        return scipy.linalg.solve(a, -0.5 * grad, assume_a="pos")
    except (np.linalg.LinAlgError, scipy.linalg.LinAlgError, ValueError):
        return np.linalg.lstsq(a, -0.5 * grad, rcond=None)[0]


def minimize(fun_and_grad, metric, x0, tol=1e-6, maxiter=500, damping=1e-6, armijo=1e-4, max_step=64.0, max_backtracks=40,
             callback=None):
    """Minimise E(theta).  ``fun_and_grad(theta) -> (E, grad)``, ``metric(theta) -> (K, K)``.  Stops when the largest gradient
    component is at most ``tol`` (success), after ``maxiter`` steps, or when the line search finds no lower energy.
    -> ``scipy.optimize.OptimizeResult`` (x, fun, jac, nit, nfev, njev, nmetric, success, status, message, energies)"""
    x = np.array(x0, dtype=np.float64).reshape(-1)
    e, g = fun_and_grad(x)
    g = np.asarray(g, np.float64).reshape(-1)
    nfev, nmetric, nit = 1, 0, 0
    energies = [float(e)]
    step = 0.5
    status, message = 1, "maximum number of iterations reached"
    while True:
        if x.size == 0 or float(np.max(np.abs(g))) <= tol:
            status, message = 0, "gradient norm below tolerance"
            break
        if nit >= maxiter:
            break
        delta = natural_step(metric(x), g, damping)
        nmetric += 1
        slope = float(g @ delta)
        if not np.all(np.isfinite(delta)) or slope >= 0.0:   # (cannot happen with a positive definite matrix; rounding at the very end)
            delta, slope = -g, -float(g @ g)
        t = min(2.0 * step, max_step)
        accepted = False
        for _ in range(max_backtracks):
            e_new, g_new = fun_and_grad(x + t * delta)
            nfev += 1
            if np.isfinite(e_new) and e_new <= e + armijo * t * slope:
                accepted = True
                break
            t *= 0.5
        if not accepted:
            status, message = 2, "line search found no lower energy"
            break
        x = x + t * delta
        e, g = e_new, np.asarray(g_new, np.float64).reshape(-1)
        step = t
        nit += 1
        energies.append(float(e))
        if callback is not None:
            callback(x)
    return scipy.optimize.OptimizeResult(x=x, fun=float(e), jac=g, nit=nit, nfev=nfev, njev=nfev, nmetric=nmetric, success=status == 0,
                                         status=status, message=message, energies=energies)
