"""Multi-start minimisation in lock-step: L-BFGS from every row of ``X0`` at once, on a function that evaluates a BATCH of points in
one call (``Statevector.energy_gradient_batch``: the exact gradients of B parameter vectors in one launch).

k-UpCCGSD and the hardware-efficient circuits are normally optimised from several random starts and the best run is kept; the
reference's ``get_energies`` runs its minimisation from two starting vectors.  Run one after the other, B starts cost B times one
start.  Here every iteration is ONE batched call on the trial points of the starts that are still active, so B starts cost about what
one does while the device has room for the batch.

Every start keeps its own state: its L-BFGS memory (``history`` pairs), its direction, its step length and its Armijo backtracking.  A
start whose trial point is rejected retries with half the step in the next call while the others move on; a start whose largest gradient
component is at most ``tol`` has converged and leaves the batch.  Nothing a start does depends on the other rows, so the run of a start
is the same alone or in company, and the whole result is a deterministic function of ``X0``.
"""
import numpy as np
import scipy.optimize


class _Start:
    """one start: the accepted point (x, f, g), the memory, and the trial in flight"""

    def __init__(self, x, f, g, history):
        self.x, self.f, self.g = x, float(f), g
        self.history = history
        self.s, self.y = [], []
        self.iterations = 0
        self.energies = [float(f)]
        self.direction = None      # None: the next trial starts a new line search
        self.slope = 0.0
        self.t = 1.0
        self.backtracks = 0
        self.status = None         # None: active; 0 converged, 1 iterations exhausted, 2 the line search found no lower energy

    def _two_loop(self):
        q = self.g.copy()
        alphas = []
        for s, y in zip(reversed(self.s), reversed(self.y)):
            a = float(s @ q) / float(y @ s)
            alphas.append(a)
            q -= a * y
        if self.s:
            q *= float(self.s[-1] @ self.y[-1]) / float(self.y[-1] @ self.y[-1])
        for (s, y), a in zip(zip(self.s, self.y), reversed(alphas)):
            b = float(y @ q) / float(y @ s)
            q += (a - b) * s
        return -q

    def trial(self):
        if self.direction is None:
            d = self._two_loop()
            slope = float(self.g @ d)
            if not np.all(np.isfinite(d)) or slope >= 0.0:   # (a memory spoilt by rounding: steepest descent, memory dropped)
                self.s, self.y = [], []
                d, slope = -self.g, -float(self.g @ self.g)
            self.direction, self.slope = d, slope
            # the first step of a start has no curvature yet: at most unit length
            self.t = 1.0 if self.s else min(1.0, 1.0 / max(float(np.linalg.norm(self.g)), 1e-300))
            self.backtracks = 0
        return self.x + self.t * self.direction

    def take(self, f_new, g_new, armijo, max_backtracks):
        """the answer for the trial point: accept it (Armijo) or halve the step"""
        if np.isfinite(f_new) and f_new <= self.f + armijo * self.t * self.slope:
            s = self.t * self.direction
            y = g_new - self.g
            sy = float(s @ y)
            if sy > 1e-10 * float(np.linalg.norm(s)) * float(np.linalg.norm(y)):
                self.s.append(s)
                self.y.append(y)
                if len(self.s) > self.history:
                    self.s.pop(0)
                    self.y.pop(0)
            self.x, self.f, self.g = self.x + s, float(f_new), g_new
            self.iterations += 1
            self.energies.append(self.f)
            self.direction = None
            return
        self.t *= 0.5
        self.backtracks += 1
        if self.backtracks >= max_backtracks:
            self.status = 2


_MESSAGES = {0: "gradient below tolerance", 1: "maximum number of iterations reached", 2: "line search found no lower energy"}


def minimize(fun_grad_batch, X0, tol=1e-6, maxiter=500, history=10, armijo=1e-4, max_backtracks=40):
    """Minimise E from every row of ``X0`` (B, K).  ``fun_grad_batch(X) -> (E[b], grad[b, K])`` for the rows of X, any number of them.
    A start stops when its largest gradient component is at most ``tol`` (converged), after ``maxiter`` accepted steps, or when its line
    search finds no lower energy.
    -> ``scipy.optimize.OptimizeResult``: the best start (lowest energy; the first of equals) as ``x``, ``fun``, ``jac``, ``nit``,
    ``success``, ``status``, ``message``, ``energies`` (its accepted energies, the starting point first) and ``best`` (its row);
    ``ncalls`` batched calls, ``rows`` rows evaluated in all; per start ``X`` (B, K), ``F``, ``G``, ``converged``, ``iterations``"""
    X0 = np.array(X0, dtype=np.float64)
    if X0.ndim == 1:
        X0 = X0[None, :]
    if X0.ndim != 2 or X0.shape[0] == 0:
        raise ValueError("X0: expected a (B, K) array with at least one row")
    B, K = X0.shape
    F, G = fun_grad_batch(X0.copy())
    F = np.asarray(F, np.float64).reshape(B)
    G = np.asarray(G, np.float64).reshape(B, K)
    ncalls, rows = 1, B
    starts = [_Start(X0[b].copy(), F[b], G[b].copy(), int(history)) for b in range(B)]

    def settle(st):
        if st.status is None:
            if K == 0 or float(np.max(np.abs(st.g))) <= tol:
                st.status = 0
            elif st.iterations >= maxiter:
                st.status = 1

    for st in starts:
        settle(st)
    while True:
        active = [st for st in starts if st.status is None]
        if not active:
            break
        F, G = fun_grad_batch(np.stack([st.trial() for st in active]))
        F = np.asarray(F, np.float64).reshape(len(active))
        G = np.asarray(G, np.float64).reshape(len(active), K)
        ncalls += 1
        rows += len(active)
        for st, f, g in zip(active, F, G):
            st.take(float(f), g.copy(), armijo, max_backtracks)
            settle(st)
    Fs = np.array([st.f for st in starts])
    best = int(np.argmin(Fs))
    top = starts[best]
    return scipy.optimize.OptimizeResult(
        x=top.x.copy(), fun=top.f, jac=top.g.copy(), nit=top.iterations, success=top.status == 0, status=top.status,
        message=_MESSAGES[top.status], energies=list(top.energies), best=best, ncalls=ncalls, rows=rows,
        X=np.stack([st.x for st in starts]), F=Fs, G=np.stack([st.g for st in starts]),
        converged=np.array([st.status == 0 for st in starts]), iterations=np.array([st.iterations for st in starts]))
