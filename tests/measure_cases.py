"""TEST INFRASTRUCTURE ONLY — checker of finite-shot measurement (ovqe_sample, ovqe_measure_paulis, ovqe_measure_groups,
ovqe_energy_sampled; include/ovqe_sv.h states the contract) and the case lists of tests/test_measure_cases.py /
tests/test_gpu_measure.py.

What is restated here, independently of the library: the basis change B (the dense one-qubit matrices of ``oracle.dense`` applied
bit by bit), the prefix sums of |phi|^2 in extended precision (numpy longdouble: 64-bit mantissa, (N - 1) 2^-64 relative for N terms),
the uniforms on Python integers, the grouping rule, and the replay of an energy estimate group by group.

ACCEPTANCE RULE of an outcome i for shot s: p_i > 0 and C_{i-1} - eps W <= u(s) W <= C_i + eps W, exact C, eps = 1e-9.  Any summation
order of N <= 2^20 non-negative doubles is within (N - 1) 2^-53 = 1.2e-10 relative of the exact sum; the butterflies and u W add a few
1e-15.  A shot whose outcome differs from the exact rule's (it lies outside the exact interval) is an EPS-MARGIN shot: at most 1 % of a
test's shots may be such (expected share <= 2 eps N <= 0.2 %)."""
import numpy as np

from oracle import dense

EPS = 1e-9
MARGIN_SHARE = 0.01
_M = (1 << 64) - 1


def mix64(v):
    v = (v + 0x9E3779B97F4A7C15) & _M
    v = ((v ^ (v >> 30)) * 0xBF58476D1CE4E5B9) & _M
    v = ((v ^ (v >> 27)) * 0x94D049BB133111EB) & _M
    return v ^ (v >> 31)


def uniforms(seed, stream, first, count):
    """u(s) for s = first .. first + count - 1, on Python integers (the product's restatement is synth.shot_uniforms)"""
    key = mix64((seed & _M) ^ mix64(stream & _M))
    return np.array([(mix64(key ^ mix64((first + k) & _M)) >> 11) / 9007199254740992.0 for k in range(count)], np.float64)


_H = dense.gate_matrix("H")
_HSDG = _H @ np.diag([1.0, -1.0j])      # H S^+: (|0> + i|1>)/sqrt 2 -> |0>


def rotate_basis(psi, n, xbasis, ybasis):
    """phi = B psi, B = (x) (H on the bits of xbasis, H S^+ on those of ybasis); index bit b is axis n - 1 - b"""
    assert not (xbasis & ybasis) and not ((xbasis | ybasis) >> n)
    phi = np.asarray(psi, np.complex128).reshape((2,) * n)
    for b in range(n):
        m = _H if (xbasis >> b) & 1 else _HSDG if (ybasis >> b) & 1 else None
        if m is not None:
            ax = n - 1 - b
            phi = np.moveaxis(np.tensordot(m, phi, axes=([1], [ax])), 0, ax)
    return np.ascontiguousarray(phi).reshape(-1)


def probabilities(psi, n, xbasis=0, ybasis=0):
    phi = rotate_basis(psi, n, xbasis, ybasis)
    return phi.real ** 2 + phi.imag ** 2


def exact_prefix(p):
    """inclusive prefix sums of p in extended precision"""
    return np.cumsum(np.asarray(p, np.longdouble))


def exact_outcomes(p, u):
    """the smallest i with C_i > u W"""
    C = exact_prefix(p)
    return np.searchsorted(C, np.asarray(u, np.longdouble) * C[-1], side="right").astype(np.uint64)


def check_outcomes(idx, p, u, what=""):
    """every outcome passes the acceptance rule -> number of eps-margin shots (asserted to stay under the 1 % cap)"""
    idx = np.asarray(idx, np.int64)
    if idx.size == 0:
        return 0
    p = np.asarray(p, np.float64)
    assert idx.min() >= 0 and idx.max() < p.size, what
    C = exact_prefix(p)
    W = C[-1]
    t = np.asarray(u, np.longdouble) * W
    below = np.where(idx > 0, C[np.maximum(idx - 1, 0)], np.longdouble(0))
    ok = (p[idx] > 0) & (below - EPS * W <= t) & (t <= C[idx] + EPS * W)
    bad = np.nonzero(~ok)[0]
    assert bad.size == 0, (what, "shots", bad[:5], "outcomes", idx[bad[:5]], "p", p[idx[bad[:5]]], "u", np.asarray(u)[bad[:5]])
    margin = int(np.count_nonzero(idx != exact_outcomes(p, u).astype(np.int64)))
    print(f"{what}: {idx.size} shots, {margin} in the eps margin")
    assert margin <= MARGIN_SHARE * idx.size, (what, margin, idx.size)
    return margin


def signs(idx, mask):
    """(-1)^popcount(b & mask) per outcome"""
    v = np.asarray(idx, np.uint64) & np.uint64(mask)
    par = np.zeros(v.shape, np.uint64)
    while v.any():
        par ^= v & np.uint64(1)
        v = v >> np.uint64(1)
    return 1 - 2 * par.astype(np.int64)


def score(idx, masks_, coeffs):
    """(term_sums int64, values per shot) of the outcomes"""
    idx = np.asarray(idx, np.uint64)
    vals = np.zeros(idx.shape[0], np.float64)
    tsum = np.zeros(len(masks_), np.int64)
    for t, (m, c) in enumerate(zip(masks_, coeffs)):
        s = signs(idx, int(m))
        tsum[t] = s.sum()
        vals += float(c) * s
    return tsum, vals


def plan_groups(xs, zs, cs):
    """the grouping rule restated: -> (group of term, xbasis per group, ybasis per group)"""
    T = len(xs)
    group = [-1] * T
    order = sorted((t for t in range(T) if int(xs[t]) | int(zs[t])), key=lambda t: (-abs(float(cs[t])), t))
    gx, gy, gz = [], [], []
    for t in order:
        x, z = int(xs[t]), int(zs[t])
        tx, ty, tz = x & ~z, x & z, z & ~x
        for g in range(len(gx)):
            if not ((tx & (gy[g] | gz[g])) | (ty & (gx[g] | gz[g])) | (tz & (gx[g] | gy[g]))):
                break
        else:
            g = len(gx)
            gx.append(0), gy.append(0), gz.append(0)
        gx[g] |= tx
        gy[g] |= ty
        gz[g] |= tz
        group[t] = g
    return np.array(group, np.int32), np.array(gx, np.uint64), np.array(gy, np.uint64)


def check_plan(n, xs, zs, cs, group, xb, yb):
    """every non-identity term is in exactly one group and agrees with its group's basis on each of its bits"""
    assert len(group) == len(xs) and len(xb) == len(yb)
    for t in range(len(xs)):
        x, z, g = int(xs[t]), int(zs[t]), int(group[t])
        if not (x | z):
            assert g == -1
            continue
        assert 0 <= g < len(xb)
        bx, by = int(xb[g]), int(yb[g])
        assert not (bx & by) and not ((bx | by) >> n)
        assert (x & ~z) & ~bx == 0 and (x & z) & ~by == 0 and (z & ~x) & (bx | by) == 0, (t, g)


def group_terms(group, g):
    return [t for t in range(len(group)) if group[t] == g]


def estimate(const, n_shots, sum_v, sum_v2):
    """energy and standard error from the groups' (sum v, sum v^2), as include/ovqe_sv.h states them"""
    e, var = float(const), 0.0
    for sv, sv2 in zip(sum_v, sum_v2):
        e += sv / n_shots
        var += max((sv2 - sv * sv / n_shots) / (n_shots - 1), 0.0)
    return e, float(np.sqrt(var / n_shots))


def replay_energy(psi, n, xs, zs, cs, const, plan, n_shots, seed):
    """the estimate of ovqe_energy_sampled replayed on the dense state with the exact rule: group g with stream g, shots 0 .. n_shots - 1
    -> (energy, std_error, outcomes per group, values per group, probabilities per group)"""
    group, xb, yb = plan
    const = float(const) + sum(float(cs[t]) for t in range(len(xs)) if not (int(xs[t]) | int(zs[t])))
    sum_v, sum_v2, outs, vals, probs = [], [], [], [], []
    for g in range(len(xb)):
        members = group_terms(group, g)
        p = probabilities(psi, n, int(xb[g]), int(yb[g]))
        idx = exact_outcomes(p, uniforms(seed, g, 0, n_shots))
        _, v = score(idx, [int(xs[t]) | int(zs[t]) for t in members], [cs[t] for t in members])
        sum_v.append(float(v.sum()))
        sum_v2.append(float((v * v).sum()))
        outs.append(idx), vals.append(v), probs.append(p)
    e, s = estimate(const, n_shots, sum_v, sum_v2)
    return e, s, outs, vals, probs


def exact_moments(psi, n, xs, zs, cs, const, plan, n_shots):
    """the estimator's exact mean (= <H>) and standard deviation sqrt(sum_g Var_g(v) / n_shots) under the exact distributions"""
    group, xb, yb = plan
    mean = float(const) + sum(float(cs[t]) for t in range(len(xs)) if not (int(xs[t]) | int(zs[t])))
    var = 0.0
    every = np.arange(1 << n, dtype=np.uint64)
    for g in range(len(xb)):
        members = group_terms(group, g)
        p = probabilities(psi, n, int(xb[g]), int(yb[g]))
        p = p / p.sum()
        _, v = score(every, [int(xs[t]) | int(zs[t]) for t in members], [cs[t] for t in members])
        m = float(p @ v)
        mean += m
        var += float(p @ (v - m) ** 2)
    return mean, float(np.sqrt(var / n_shots))


# ---- states of the sampling tests -------------------------------------------------------------------------------------------------
def spike_states(n):
    """{name: state}: basis states at both ends, two spikes with W != 1, a weight that ends mid-block with zeros behind it"""
    N = 1 << n
    out = {}
    for name, i in (("first", 0), ("last", N - 1)):
        psi = np.zeros(N, np.complex128)
        psi[i] = 1.0
        out[name] = psi
    psi = np.zeros(N, np.complex128)
    psi[0], psi[N - 1] = 0.6 + 0.3j, -1.1j
    out["two spikes"] = psi
    psi = np.zeros(N, np.complex128)
    end = max(1, (N * 5) // 8 - 3) if N > 8 else max(1, N // 2)
    rng = np.random.default_rng(n)
    psi[:end] = rng.normal(size=end) + 1j * rng.normal(size=end)
    psi[rng.integers(0, end, max(1, end // 4))] = 0.0      # holes inside the weight too
    psi[end - 1] = 0.5
    out["mid-block tail"] = psi
    return out


# ---- inputs of the energy_sampled replay tests --------------------------------------------------------------------------------------
class EnergyCase:
    """n, Hamiltonian, a program (UCC generators or a literal gate list), theta and the seed of the shots"""

    def __init__(self, name, n, ham, hf, theta, seed, gens=None, gates=None):
        self.name, self.n, self.ham, self.hf, self.theta, self.seed, self.gens, self.gates = name, n, ham, int(hf), np.asarray(theta, float), seed, gens, gates

    def load(self, sv):
        sv.set_hamiltonian(self.ham)
        if self.gens is not None:
            sv.set_ucc_program(self.gens, self.hf)
        else:
            sv.set_gate_program(self.gates, len(self.theta), self.hf)

    def packed(self):
        from openvqe_amd.operators import pack_terms
        xs, zs, cs = pack_terms(self.n, self.ham.terms)
        return xs, zs, np.ascontiguousarray(cs.real), complex(self.ham.constant_coeff or 0.0).real


def energy_case(name):
    import json
    import os

    from openvqe_amd import chem, fermion
    from openvqe_amd.operators import Hamiltonian, Term
    from tests import util
    if name == "H2":
        k1 = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "k1_h2_sto3g.json")))
        ham = Hamiltonian(4, [Term(c, o, q) for c, o, q in k1["terms"]], k1["constant_coeff"])
        return EnergyCase(name, 4, ham, k1["hf_init"], [0.05, -0.03, -0.1137], 1, gens=fermion.uccsd_generators(2, 1))
    if name == "LiH":
        mol = chem.molecule("LiH")
        mol.rhf()
        ham = mol.jw_hamiltonian()
        n = ham.nbqbits
        hf = mol.hf_init()
        hf = int(hf) if np.isscalar(hf) else int(sum(1 << (n - 1 - q) for q, v in enumerate(hf) if v))
        gens = fermion.uccsd_generators(mol.nao, mol.n_elec // 2)
        return EnergyCase(name, n, ham, hf, np.random.default_rng(12).uniform(-0.2, 0.2, len(gens)), 1, gens=gens)
    if name == "random8":
        rng = np.random.default_rng(88)
        ham = util.random_hamiltonian(rng, 8, 40)
        gates, K = util.quccsd_like_gates(rng, 8, 3, 2, extra_random=6)
        return EnergyCase(name, 8, ham, 0b11000000, rng.uniform(-0.7, 0.7, K), 3, gates=gates)
    raise KeyError(name)
