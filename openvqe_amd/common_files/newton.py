"""Newton trust-region minimisation of the energy of a parameterised state, and the stability check of a converged point — the
second-order siblings (scipy's ``trust-exact``) of the ``scipy.optimize.minimize`` calls the reference makes.

``Statevector.energy_hessian`` answers E, the exact gradient and the exact Hessian of one point in one device call; scipy asks for the
three through separate callbacks, so one call per iterate is cached by the bytes of theta.  ``trust-exact`` solves the trust-region
subproblem from the eigenvalues of the Hessian: it steps along directions of negative curvature, so it leaves the saddle points a
quasi-Newton method can stop at, and it accepts a trial point only when the energy falls — the accepted energies never rise.
"""
import numpy as np
import scipy.optimize


def stability(hess):
    """(lowest eigenvalue, its eigenvector) of the symmetric part of ``hess``: a converged point is a minimum when the eigenvalue is not
    negative, and the eigenvector is the direction to leave a saddle along"""
    h = np.asarray(hess, np.float64)
    if h.size == 0:
        return 0.0, np.zeros(0)
    vals, vecs = np.linalg.eigh(0.5 * (h + h.T))
    return float(vals[0]), vecs[:, 0].copy()


def minimize(fun_grad_hess, x0, tol=1e-6, maxiter=500, callback=None):
    """Minimise E(theta).  ``fun_grad_hess(theta) -> (E, grad, hess)``, called once per distinct theta.  Stops when the 2-norm of the
    gradient (hence its largest component) is at most ``tol``.
    -> ``scipy.optimize.OptimizeResult`` of ``trust-exact`` plus ``energies`` (E at x0 and at every accepted iterate: non-increasing),
    ``ncalls`` (device calls), ``lowest_eigenvalue`` of the Hessian at the solution"""
    x0 = np.array(x0, dtype=np.float64).reshape(-1)
    cache = {}
    ncalls = [0]

    def at(theta):
        key = np.ascontiguousarray(theta, np.float64).tobytes()
        hit = cache.pop(key, None)
        if hit is not None:
            cache[key] = hit   # (most recently used last)
        else:
            e, g, h = fun_grad_hess(np.array(theta, dtype=np.float64))
            hit = (float(e), np.array(g, dtype=np.float64).reshape(-1), np.array(h, dtype=np.float64))
            if len(cache) >= 2:   # (the current iterate and the trial point: scipy asks for fun, jac and hess of either in a row)
                cache.pop(next(iter(cache)))
            cache[key] = hit
            ncalls[0] += 1
        return hit

    energies = [at(x0)[0]]

    def on_iterate(xk, *_):
        energies.append(at(xk)[0])
        if callback is not None:
            callback(xk)

    if x0.size == 0:
        return scipy.optimize.OptimizeResult(x=x0, fun=energies[0], jac=np.zeros(0), hess=np.zeros((0, 0)), nit=0, success=True, status=0,
                                             message="no parameters", energies=energies, ncalls=ncalls[0], lowest_eigenvalue=0.0)
    res = scipy.optimize.minimize(lambda t: at(t)[0], x0, jac=lambda t: at(t)[1], hess=lambda t: at(t)[2], method="trust-exact",
                                  callback=on_iterate, options={"gtol": tol, "maxiter": maxiter})
    e, g, h = at(res.x)
    res.fun, res.jac, res.hess = e, g, h
    res.energies = energies
    res.ncalls = ncalls[0]
    res.lowest_eigenvalue = stability(h)[0]
    return res
