"""TEST INFRASTRUCTURE ONLY — the batched exact gradient (ovqe_energy_gradient_batch): the checker, the bounds, a Python restatement of
the kernel's LDS layout (sp_grad_batch_lds, csrc/sv_sparse_layout.hpp) and of the launch planner (csrc/sv_gradbatch_host.hpp), and the
case builders of tests/test_gradbatch_cases.py / tests/test_gpu_gradient_batch.py.

The checker is ``oracle.masks.ucc_energy_gradient``: the adjoint pass on the dense complex register, no finite differences."""
import numpy as np

from oracle import masks
from tests import hessian_cases
from tests.util import cascade_geometry, compile_generators, pattern_excitation, y_rotation

LDS_BUDGET = 150 * 1024    # LDS_WG_BUDGET: what a candidate may take
LDS_CU = 160 * 1024        # the LDS of a CU
WAVES_CU = {True: 28, False: 24}   # the waves a CU holds of the staged / unstaged instances (72 / 73 VGPRs: 7 / 6 per SIMD)
WAVES = (1, 2, 4, 8)


# ---- bounds -------------------------------------------------------------------------------------------------------------------------------
def bound_checker(h1, C):
    """against the checker: the project's 1e-10 ||H||_1 energy bound carried through one derivative (``test_gpu_hessian`` holds E and
    the gradient of ``energy_hessian`` to it)"""
    return 1e-10 * h1 * max(1.0, C)


def bound_single(h1, C):
    """against ``energy_gradient`` of the same handle"""
    return 1e-12 * h1 * max(1.0, C)


# ---- the kernel's LDS and the planner's rule, restated -----------------------------------------------------------------------------------
def slots(m):
    """the compact state of a support of m basis states: the planner of the energy paths (csrc/sparse_plan.hpp) numbers a support of
    33 to 4064 states into rows of 32 slots; smaller and larger ones keep their discovery order"""
    return (m + 31) // 32 * 32 if 32 < m <= 4064 else m


def wave_stride(m, ntab, K):
    """one wave's region (m: the SLOTS of the state): psi and lambda ([mpad] doubles, mpad = m rounded up to even), cos / sin (16 bytes) and w (8 bytes) per table
    entry, gk ([K] doubles, K rounded up to even) — the unstaged layout of the single kernel — rounded up to 16 bytes"""
    mpad = (m + 1) & ~1
    return (2 * mpad * 8 + ntab * 24 + ((K + 1) & ~1) * 8 + 15) & ~15


def batch_lds_bytes(m, ntab, nops, npairs, K, nw, stage):
    """nw regions, and behind them — staged — ONE copy of the 16-byte op records and of the 4-byte pair words"""
    return nw * wave_stride(m, ntab, K) + (nops * 16 + npairs * 4 if stage else 0)


def eligible(m, ntab, K):
    return wave_stride(m, ntab, K) <= LDS_BUDGET


def plan(m, ntab, nops, npairs, K, B, waves=0, workgroups=0, cus=256):
    """the planner's choice -> dict(nw, stage, per_cu, workgroups, lds), or None when no candidate is admissible: most resident waves
    per CU, min(LDS_CU // bytes, WAVES_CU[stage] // nw) * nw; ties: staged first, then the smaller nw.  ``waves`` restricts the candidates to
    one nw; where none of those is admissible the choice is the automatic one"""
    if waves in WAVES and batch_lds_bytes(m, ntab, nops, npairs, K, waves, False) > LDS_BUDGET:
        waves = 0
    best = None
    for stage in (True, False):
        for nw in WAVES:
            if waves in WAVES and nw != waves:
                continue
            nbytes = batch_lds_bytes(m, ntab, nops, npairs, K, nw, stage)
            if nbytes > LDS_BUDGET:
                continue
            per_cu = min(LDS_CU // nbytes, WAVES_CU[stage] // nw)
            if best is None or per_cu * nw > best["per_cu"] * best["nw"]:
                best = dict(nw=nw, stage=stage, per_cu=per_cu, lds=nbytes)
    if best is None:
        return None
    wgs = min(-(-B // best["nw"]), max(cus, 1) * best["per_cu"])
    if workgroups > 0:
        wgs = min(wgs, workgroups)
    best["workgroups"] = max(wgs, 1)
    return best


def check_info(info, sizes, B, waves=0, workgroups=0, cus=None):
    """``gradient_batch_info()`` of a path-1 call against the restated rule; ``sizes`` = (slots, ntab, nops, npairs, K).  Without ``cus``
    the grid is checked where it does not depend on the device: it is the rows' or the cap's"""
    m, ntab, nops, npairs, K = sizes
    want = plan(m, ntab, nops, npairs, K, B, waves, workgroups, cus if cus else 1 << 20)
    assert want is not None and info["path"] == 1 and info["launches"] == 1, (info, want)
    assert (info["B"], info["K"]) == (B, K) and slots(info["support"]) == m, (info, sizes)
    assert info["waves"] == want["nw"] and info["form"] == (1 if want["stage"] else 2) and info["lds_bytes"] == want["lds"], (info, want)
    if cus or want["workgroups"] <= 8:
        assert info["workgroups"] == want["workgroups"], (info, want)
    else:
        assert 1 <= info["workgroups"] <= want["workgroups"], (info, want)
    return want


# ---- cases -------------------------------------------------------------------------------------------------------------------------------
class Case:
    """a rotation program (index-bit masks) with a real Hamiltonian, and the checker's answers, computed once per parameter vector"""

    def __init__(self, n, hf, rx, rz, rc, pidx, K, phi0=None, nterms=16, seed=1, ham=None):
        self.n, self.hf, self.K, self.phi0 = int(n), int(hf), int(K), phi0
        self.rx, self.rz = np.ascontiguousarray(rx, np.uint64), np.ascontiguousarray(rz, np.uint64)
        self.rc, self.pidx = np.ascontiguousarray(rc, np.float64), np.ascontiguousarray(pidx, np.int32)
        if ham is None:
            hx, hz, hc = hessian_cases.random_real_hamiltonian(n, nterms, seed, x_pool=self.rx[:64])
            self.h = (hx, hz, hc, 0.25)
            self.ham = hessian_cases.hamiltonian_object(n, hx, hz, hc, 0.25)
        else:
            from openvqe_amd.operators import pack_terms
            hx, hz, hc = pack_terms(n, ham.terms)
            self.h = (hx, hz, np.real(hc), float(np.real(ham.constant_coeff or 0.0)))
            self.ham = ham
        self.h1 = hessian_cases.norm1(self.h[2], self.h[3])
        self.C = hessian_cases.coefficient_sum(self.rc, self.pidx, self.K)
        self._want = {}

    def load(self, sv):
        sv.set_hamiltonian(self.ham)
        sv.set_rotation_program(self.rx, self.rz, self.rc, self.pidx, self.K, self.hf, phi0=self.phi0)

    def want(self, theta):
        """(E, grad[K]) of the checker"""
        theta = np.ascontiguousarray(theta, np.float64)
        key = theta.tobytes()
        if key not in self._want:
            self._want[key] = masks.ucc_energy_gradient(self.n, self.hf, self.rx, self.rz, self.rc, self.pidx, theta, *self.h, self.phi0)
        return self._want[key]

    def tol_checker(self):
        return bound_checker(self.h1, self.C)

    def tol_single(self):
        return bound_single(self.h1, self.C)


def from_generators(n, hf, gens, K, seed):
    rx, rz, rc, rp = compile_generators(gens)
    return Case(n, hf, rx, rz, rc, rp, K, seed=seed)


def no_active_op():
    """m = 1: the only generator moves amplitude between two bits that are both empty in |hf> — no pair on the support, the derivative
    an exact zero -> (case, (m, nops, npairs, K))"""
    case = from_generators(4, 1, [pattern_excitation([2], [3]) + (0,)], 1, seed=31)
    return case, (1, 0, 0, 1)


def two_states():
    """m = 2: one Y rotation"""
    n, hf, gens, K = cascade_geometry(1, 0, 0)
    case = from_generators(n, hf, gens, K, seed=32)
    return case, (2, 1, 1, 1)


def per_rotation(K):
    """K rotations with a parameter each: Y round the seven index bits from |0...0> (m = 128 from the seventh on).  Consecutive
    rotations differ in their x masks: a run that shares x but not the parameter is no op of the compact program"""
    gens = [y_rotation(r % 7) + (r,) for r in range(K)]
    rx, rz, rc, rp = compile_generators(gens)
    rc = rc * np.random.default_rng(K).uniform(0.5, 1.5, K)
    return Case(7, 0, rx, rz, rc, rp, K, nterms=20, seed=300 + K)


# m = 4096 on 12 qubits: Y on every index bit from |0...0>, then the Y rotations again, round the bits, up to R rotations: every rotation
# past the twelfth is one op of 2048 pairs and one table entry; the parameters go round Y_K of them
Y_N, Y_K = 12, 24


def y_sizes(R, n=Y_N):
    """(slots, ntab, nops, npairs, K) of ``y_program(R, n)``: the j-th of the first n rotations pairs the 2^j states so far with new ones"""
    assert R >= n
    return slots(1 << n), R, R, (1 << n) - 1 + (R - n) * (1 << (n - 1)), Y_K


def y_program(R, seed=4096, n=Y_N):
    gens = [y_rotation(r % n) + (r % Y_K,) for r in range(R)]
    rx, rz, rc, rp = compile_generators(gens)
    rc = rc * np.random.default_rng(seed).uniform(0.5, 1.0, R)   # (distinct magnitudes: a table entry per rotation)
    return Case(n, 0, rx, rz, rc, rp, Y_K, nterms=16, seed=seed)


# 1024 states, 30 rotations: eight regions of 17 KiB fit the budget, the 45 KiB of pair words beside them do not
EIGHT_PLAIN = (30, 10)


def y_boundaries():
    """R on both sides of every decision the layout makes at m = 4096, from the restated formula.  One wave's region is 64 KiB and 24
    bytes per rotation, so a CU holds two of them — as one workgroup of two waves or as two workgroups of one — up to ``two_last``:
    ``two_staged`` / ``two_plain``: automatic — the last program that runs two waves per workgroup (the staged form wins the tie with
        two unstaged one-wave workgroups) and the first whose pair words no longer fit beside two regions: one wave, unstaged;
        (a staged one-wave form never runs at this support: two unstaged one-wave workgroups per CU beat its one);
    ``two_last`` / ``one_first``: under "grad_batch_waves" = 2, the last program two regions fit the budget for and the first that is
        planned as if the option were not set;
    ``path1_last`` / ``path2_first``: the last program one region fits the budget for and the first that falls to path 2"""
    auto = lambda R: plan(*y_sizes(R), 3)   # noqa: E731
    one = lambda R: plan(*y_sizes(R), 3, waves=1)   # noqa: E731
    two = lambda R: plan(*y_sizes(R), 3, waves=2)   # noqa: E731
    out = {}
    R = Y_N
    assert auto(R)["nw"] == 2 and auto(R)["stage"]
    while auto(R + 1)["nw"] == 2:
        R += 1
    out["two_staged"], out["two_plain"] = R, R + 1
    assert (auto(R + 1)["nw"], auto(R + 1)["stage"], auto(R + 1)["per_cu"]) == (1, False, 2)
    assert (one(Y_N)["stage"], one(Y_N)["per_cu"]) == (False, 2)
    lo, hi = out["two_plain"], 1 << 14          # (the layouts grow with R: bisection)
    assert two(lo)["nw"] == 2 and not two(lo)["stage"] and auto(hi) is None
    while hi - lo > 1:
        mid = (lo + hi) // 2
        p = two(mid)
        lo, hi = (mid, hi) if p is not None and p["nw"] == 2 else (lo, mid)
    out["two_last"], out["one_first"] = lo, hi
    assert two(hi) == auto(hi) and two(hi)["nw"] == 1
    lo, hi = out["one_first"], 1 << 14
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if auto(mid) is not None else (lo, mid)
    out["path1_last"], out["path2_first"] = lo, hi
    assert eligible(*[y_sizes(lo)[k] for k in (0, 1, 4)]) and not eligible(*[y_sizes(hi)[k] for k in (0, 1, 4)])
    return out


# (R, "grad_batch_waves", expected nw, expected form) of the GPU boundary cases; form 0: path 2
def y_boundary_cases():
    b = y_boundaries()
    return [(b["two_staged"], 0, 2, 1), (b["two_plain"], 0, 1, 2),
            (b["two_last"], 2, 2, 2), (b["one_first"], 2, 1, 2), (b["path1_last"], 0, 1, 2), (b["path2_first"], 0, 0, 0)]
