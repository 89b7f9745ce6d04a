"""Shared helpers for the tests: seeded random Pauli operators / programs."""
import numpy as np

from openvqe_amd.operators import Hamiltonian, Term


def random_string(rng, n, min_weight=1, max_weight=None, alphabet="XYZ"):
    max_weight = max_weight or n
    w = int(rng.integers(min_weight, max_weight + 1))
    qs = sorted(rng.choice(n, w, replace=False).tolist())
    op = "".join(rng.choice(list(alphabet), w))
    return op, qs


def random_hamiltonian(rng, n, nterms, constant=None):
    seen = set()
    terms = []
    while len(terms) < nterms:
        op, qs = random_string(rng, n)
        key = (op, tuple(qs))
        if key in seen:
            continue
        seen.add(key)
        terms.append(Term(float(rng.normal()), op, qs))
    return Hamiltonian(n, terms, float(rng.normal()) if constant is None else constant)


def random_generators(rng, n, k, max_terms=4, same_support_prob=0.5):
    """k Hermitian generators with real coefficients; some share an x-mask inside (fusable runs)."""
    gens = []
    for _ in range(k):
        nt = int(rng.integers(1, max_terms + 1))
        terms = []
        if rng.random() < same_support_prob:
            # strings on one support differing in X<->Y only: identical x masks
            w = int(rng.integers(1, min(n, 4) + 1))
            qs = sorted(rng.choice(n, w, replace=False).tolist())
            for _ in range(nt):
                op = "".join(rng.choice(list("XY"), w))
                terms.append(Term(float(rng.normal()), op, qs))
        else:
            for _ in range(nt):
                op, qs = random_string(rng, n)
                terms.append(Term(float(rng.normal()), op, qs))
        gens.append(Hamiltonian(n, terms, do_clean_up=False))
    return gens


def random_state(rng, n):
    psi = rng.normal(size=1 << n) + 1j * rng.normal(size=1 << n)
    return psi / np.linalg.norm(psi)


def quccsd_like_gates(rng, n, n_single, n_double, extra_random=0, disjoint_ladders=False):
    """literal gate list of the reference's fermionic QUCCSD templates on random excitations (traced through
    openvqe_amd.common_files.circuit with symbolic angles) + optional random literal gates.
    -> (gates [(name, qubits, scale, const, pidx)], K)"""
    from openvqe_amd.common_files.circuit import efficient_fermionic_ansatz
    from openvqe_amd.qat_compat import AffineParam, Program, lower_circuit
    exci = []
    for _ in range(n_single):
        a, b = sorted(rng.choice(n, 2, replace=False).tolist())
        exci.append([a, b])
    for _ in range(n_double):
        q = rng.choice(n, 4, replace=False).tolist()
        # occupied pair below the virtual pair (the UCCSD index order) keeps the two CNOT ladders apart; interleaved
        # ladders, which the reference's ladder code does not undo exactly, otherwise
        exci.append(sorted(q) if disjoint_ladders else sorted(q[:2]) + sorted(q[2:]))
    order = rng.permutation(len(exci))
    exci = [exci[i] for i in order]
    K = len(exci)
    prog = Program()
    reg = prog.qalloc(n)
    efficient_fermionic_ansatz(reg, prog, exci, [AffineParam(k) for k in range(K)])
    _, kind, gates = lower_circuit(prog.to_circ())
    assert kind == "gates"
    gates = list(gates)
    for _ in range(extra_random):
        name = str(rng.choice(["X", "H", "RX", "RY", "RZ", "CNOT"]))
        pos = int(rng.integers(0, len(gates) + 1))
        if name == "CNOT":
            c, t = rng.choice(n, 2, replace=False).tolist()
            g = (name, [c, t], 0.0, 0.0, -1)
        elif name in ("X", "H"):
            g = (name, [int(rng.integers(0, n))], 0.0, 0.0, -1)
        else:
            g = (name, [int(rng.integers(0, n))], float(rng.choice([1.0, -1.0, -2.0])), float(rng.uniform(-1, 1)),
                 int(rng.integers(-1, K)))
        gates.insert(pos, g)
    return gates, K


# ---- support geometry of real-amplitude rotation programs (index-bit masks: bit b of a basis index is qubit n-1-b) ----------------
def y_rotation(bit):
    """one Y string on index bit ``bit``: (xs, zs, coeffs) — doubles every support it acts on"""
    return [1 << bit], [1 << bit], [1.0]


def pattern_excitation(occ, virt, chain=()):
    """(xs, zs, coeffs) of G = i(T - T^+), T = |virt occupied, occ empty><occ occupied, virt empty| on the bits occ + virt (index
    bits), times Z on the ``chain`` bits: the JW excitation without (or with a given) parity chain.  exp(-i theta G) is real; it
    moves amplitude only between basis states whose bits occ + virt read all-ones / all-zeros in either of the two matching ways.
    2^(w-1) strings of odd Y count with coefficients +-2^(1-w) (w = |occ| + |virt|)."""
    bits = list(occ) + list(virt)
    sign = {b: 1 for b in occ}            # T = prod_occ (X + iY)/2 prod_virt (X - iY)/2
    sign.update({b: -1 for b in virt})
    w = len(bits)
    x = sum(1 << b for b in bits)
    zc = sum(1 << b for b in chain)
    xs, zs, cs = [], [], []
    for sel in range(1 << w):             # Y on the selected bits, X elsewhere; only odd counts survive in T - T^+
        ys = [bits[k] for k in range(w) if (sel >> k) & 1]
        if len(ys) % 2 == 0:
            continue
        s = 1
        for b in ys:
            s *= sign[b]
        # i (T - T^+) = 2^(1-w) sum_{|S| odd} (prod s_b) i^(|S|+1) P_S
        xs.append(x)
        zs.append(sum(1 << b for b in ys) | zc)
        cs.append(float(s * (1 if (len(ys) + 1) % 4 == 0 else -1)) * 2.0 ** (1 - w))
    return xs, zs, cs


def compile_generators(gens):
    """[(xs, zs, coeffs, pidx), ...] -> rotation arrays (rx, rz, rc, pidx) in order"""
    rx = np.array([x for g in gens for x in g[0]], np.uint64)
    rz = np.array([z for g in gens for z in g[1]], np.uint64)
    rc = np.array([c for g in gens for c in g[2]], np.float64)
    rp = np.array([g[3] for g in gens for _ in g[0]], np.int32)
    return rx, rz, rc, rp


def support_closure(hf_index, rx, rz, rc, pidx):
    """Reachable support of |hf> under the rotation list, for generic angles: runs of consecutive rotations with one x mask commute
    (odd Y counts) and act on each pair (i, i ^ x) with the angle sum_r rc_r theta_{pidx_r} <i ^ x| P_r |i>, so a pair is touched
    unless that linear form is identically zero.  -> sorted uint64 array of basis indices."""
    S = np.array([int(hf_index)], np.uint64)
    r, R = 0, len(rx)
    while r < R:
        x = int(rx[r])
        e = r
        while e < R and int(rx[e]) == x:
            e += 1
        if x:
            pivot = 1 << (x.bit_length() - 1)
            i0 = np.where(S & np.uint64(pivot), S ^ np.uint64(x), S)
            i0 = np.unique(i0)
            form = {}
            for t in range(r, e):
                z = int(rz[t])
                ny = bin(x & z).count("1")
                par = _parity64(i0 & np.uint64(z))
                amp = float(rc[t]) * (1j ** (ny % 4)) * (1.0 - 2.0 * par)
                form[int(pidx[t])] = form.get(int(pidx[t]), 0.0) + amp
            active = np.zeros(i0.shape[0], bool)
            for v in form.values():
                active |= v != 0
            S = np.union1d(S, np.concatenate([i0[active], i0[active] ^ np.uint64(x)]))
        r = e
    return S


def _parity64(v):
    v = v.copy()
    for s in (32, 16, 8, 4, 2, 1):
        v ^= v >> np.uint64(s)
    return (v & np.uint64(1)).astype(np.float64)


def cascade_geometry(k, t, d, first_param=0):
    """Generators on index bits 0 .. k + d whose support has exactly (2^(k+1) - 2^(k-t)) * 2^d basis states from |hf> = bit 0:
    Y on bits 1..k (2^k states, bit 0 set), then the single excitations bit 0 -> bit j, j = 1..t (the j-th adds 2^(k-j): states
    with bit 0 set and bit j clear whose partner is new), then Y on bits k+1 .. k+d (a factor 2^d).  t = k: 2^(k+1) - 1.
    -> (n_bits, hf_index, [(xs, zs, coeffs, pidx)], K)"""
    gens, p = [], first_param
    for b in range(1, k + 1):
        gens.append(y_rotation(b) + (p,))
        p += 1
    for j in range(1, t + 1):
        gens.append(pattern_excitation([0], [j]) + (p,))
        p += 1
    for b in range(k + 1, k + d + 1):
        gens.append(y_rotation(b) + (p,))
        p += 1
    return k + d + 1, 1, gens, p - first_param
