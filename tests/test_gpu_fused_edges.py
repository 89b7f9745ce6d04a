"""The fused whole-circuit kernel (k_small_vqe, sv_small.hpp) at its structural boundaries, every handle under force_path = 1.

Reference: the mask oracle (oracle/masks.py, numpy complex128) on the same rotation list / gate list.  Tolerance: the project's
contract |E - E_ref| < 1e-10 * max(1, |H|_1).  Two launches that run the same instructions on the same inputs must agree bit for
bit (the kernel has no atomics and its block sum reduces in a fixed order): repeated parameter rows, mapped against staged I/O,
host against device entry.

Every case asserts, through Statevector.fused_launch() (ovqe_last_support which = 8..13), that the launch it is about took place
in the form it names.  The kernel returns energies only, so the programs leave dense states (a first layer touching every qubit)
and each case is read through several Hamiltonians set in turn: a random one, the sum of the single-qubit Z, one X string on all
qubits (and, on particle-conserving states, hopping + diagonal terms inside the sector).

Segment counts are compared with the rule written down in rebuild_small_program's contract: a segment closes when the next op's
table entries would pass 512 or when it holds 192 ops.  Gate programs of 191 / 192 / 193 / 385 ops: one segment up to 192 ops; at
193 the second segment holds one literal gate and no table entry; at 385 the middle segment is 192 literal gates (a stretch of
more than 192 X / H / CNOT gates exists only there: the shorter programs cannot hold one).
"""
import numpy as np
import pytest

from oracle import dense, masks
from openvqe_amd.operators import Hamiltonian, Term
from tests.util import pattern_excitation

pytestmark = pytest.mark.gpu

TOL = 1e-10
CS_CAP = 512      # entries of the LDS cos/sin table
OPS_CAP = 192     # ops of a segment
STAGE_CAP = 682   # expectation terms the idle table stages: 512 * 32 B / 24 B
IO_DOUBLES = 131072


@pytest.fixture(scope="module")
def SV(gpu_lib):
    from openvqe_amd.backend import Statevector
    return Statevector


# ---------------------------------------------------------------------------------------------------------------- helpers
class MaskHam:
    """Hermitian Pauli sum in index-bit masks (oracle/masks.py convention) + the operator object the backend takes"""

    def __init__(self, n, xs, zs, cs, const=0.0):
        self.n = n
        self.xs = [int(x) for x in xs]
        self.zs = [int(z) for z in zs]
        self.cs = np.array(cs, np.float64)
        self.const = float(const)
        self.scale = max(1.0, float(np.abs(self.cs).sum()))
        terms = []
        for x, z, c in zip(self.xs, self.zs, self.cs):
            op, qs = [], []
            for b in range(n - 1, -1, -1):
                xb, zb = (x >> b) & 1, (z >> b) & 1
                if xb or zb:
                    op.append("Y" if xb and zb else ("X" if xb else "Z"))
                    qs.append(n - 1 - b)
            terms.append(Term(float(c), "".join(op), qs))
        self.op = Hamiltonian(n, terms, self.const, do_clean_up=False)

    def expectation(self, psi):
        return masks.expectation(psi, self.xs, self.zs, self.cs, self.const)


def random_ham(rng, n, nterms=16):
    """distinct non-identity strings; a few x masks are shared, so x-groups hold several terms"""
    nterms = min(nterms, 4 ** n - 1)
    pool = [0] + [int(v) for v in rng.integers(1, 1 << n, 5)]
    seen = set()
    while len(seen) < nterms:
        x = pool[int(rng.integers(len(pool)))] if rng.random() < 0.6 else int(rng.integers(0, 1 << n))
        z = int(rng.integers(0, 1 << n))
        if x or z:
            seen.add((x, z))
    seen = sorted(seen)
    return MaskHam(n, [s[0] for s in seen], [s[1] for s in seen], rng.normal(size=len(seen)), float(rng.normal()))


def z_sum(n):
    return MaskHam(n, [0] * n, [1 << b for b in range(n)], [1.0] * n)


def wide_x(n):
    return MaskHam(n, [(1 << n) - 1], [0], [1.0])


def standard_hams(rng, n):
    return [random_ham(rng, n), z_sum(n), wide_x(n)]


class Prog:
    """rotation list exp(-i (c theta[p] + phi0) P), first rotation first"""

    def __init__(self, n, hf, K):
        self.n, self.hf, self.K = n, int(hf), K
        self.rx, self.rz, self.rc, self.rp, self.phi0 = [], [], [], [], []
        self._cache = {}

    def add(self, x, z, c, p, phi0=0.0):
        self.rx.append(int(x)); self.rz.append(int(z)); self.rc.append(float(c)); self.rp.append(int(p)); self.phi0.append(float(phi0))

    def install(self, sv):
        sv.set_rotation_program(self.rx, self.rz, self.rc, self.rp, self.K, self.hf, self.phi0)

    def state(self, theta):
        key = np.asarray(theta, np.float64).tobytes()
        if key not in self._cache:
            self._cache[key] = masks.ucc_state(self.n, self.hf, self.rx, self.rz, self.rc, self.rp, theta, self.phi0)
        return self._cache[key]

    def is_real(self):
        return all(bin(x & z).count("1") & 1 for x, z in zip(self.rx, self.rz))

    def runs(self):
        """lengths of the runs of consecutive rotations with one x mask: one op of the sequential program each"""
        out = []
        for r, x in enumerate(self.rx):
            if r and x == self.rx[r - 1]:
                out[-1] += 1
            else:
                out.append(1)
        return out


def odd_y_string(rng, n):
    x = int(rng.integers(1, 1 << n))
    z = int(rng.integers(0, 1 << n))
    if not bin(x & z).count("1") & 1:
        z ^= x & -x
    return x, z


def dense_layer(P, rng, real, params, phi0=False):
    """a rotation on every qubit with generic angles: every amplitude of the register is populated behind it; complex mode adds an
    X rotation per qubit, so the amplitudes are complex.  phi0: constant parts too (such a rotation is no table op)"""
    for b in range(P.n):
        P.add(1 << b, 1 << b, rng.uniform(0.5, 1.5), params[b % len(params)] if params else -1,
              rng.uniform(0.2, 1.0) if (phi0 or not params) else 0.0)
        if not real:
            P.add(1 << b, 0, rng.uniform(0.5, 1.5), params[(b + 1) % len(params)] if params else -1, rng.uniform(0.2, 1.0))


def entanglers(P, rng, real, count, params):
    for _ in range(count):
        if real:
            x, z = odd_y_string(rng, P.n)
        else:
            x, z = int(rng.integers(0, 1 << P.n)), int(rng.integers(0, 1 << P.n))   # x = 0: a diagonal run
            if not (x or z):
                z = 1
        P.add(x, z, rng.uniform(-1, 1), params[int(rng.integers(len(params)))] if params else -1,
              0.0 if (real and params) else rng.uniform(-0.5, 0.5))


def dense_program(rng, n, real, K, hf, n_ent=6):
    P = Prog(n, hf, K)
    params = list(range(K))
    dense_layer(P, rng, real, params)
    if n > 1:
        entanglers(P, rng, real, n_ent, params)
    return P


def lds_state(n, real):
    return n <= (14 if real else 13)


def threads(n, real):
    if not lds_state(n, real):
        return 1024
    return 64 if n <= 8 else (256 if n <= 10 else 1024)


def io_form(B, K, poll=True, device=False):
    if device:
        return "device"
    if B <= 1024 and B * (K + 1) <= IO_DOUBLES:
        return "polled" if (B <= 256 and poll) else "mapped"
    return "staged"


def assert_launch(sv, n, real, B, K, poll=True, device=False):
    """the last launch was the fused kernel, in the instance and I/O form the shape calls for"""
    f = sv.fused_launch()
    assert f["launched"], "no fused launch: the call was served by another path"
    assert f["real"] == real, f
    assert f["lds_state"] == lds_state(n, real), f
    assert f["threads"] == threads(n, real), f
    assert f["workgroups"] == min(B, 1024 if lds_state(n, real) else 512), f
    io = io_form(B, K, poll, device)
    assert f["mapped_io"] == (io in ("polled", "mapped")), (io, f)
    assert f["polled"] == (io == "polled"), (io, f)
    assert f["device_entry"] == (io == "device"), (io, f)
    return f


def check_rows(e, rows, thetas, state_of, H, what=""):
    for b in sorted(set(rows)):
        ref = H.expectation(state_of(thetas[b]))
        assert abs(e[b] - ref) < TOL * H.scale, (what, b, e[b], ref)


def expected_segments(entries):
    """entries[o]: table entries of op o of the fused program (0: literal gate)"""
    segs = ops_in = ent_in = 0
    for e in entries:
        if ops_in and (ops_in >= OPS_CAP or ent_in + e > CS_CAP):
            segs += 1
            ops_in = ent_in = 0
        ops_in += 1
        ent_in += e
    return segs + (1 if ops_in else 0)


def split_runs(runs):
    """runs of the sequential program that are no table ops -> entries per op of the fused program (runs longer than the table split)"""
    out = []
    for r in runs:
        while r > CS_CAP:
            out.append(CS_CAP)
            r -= CS_CAP
        out.append(r)
    return out


# ------------------------------------------------------------------------------------------------------------- batch wrap
def _wrap_case(SV, n, real, B, grid):
    rng = np.random.default_rng(1000 + 10 * n + real)
    K = 3
    P = dense_program(rng, n, real, K, hf=int(rng.integers(0, 1 << n)), n_ent=5)
    assert P.is_real() == real
    base = rng.uniform(-1, 1, (grid, K))
    thetas = base[np.arange(B) % grid]
    rows = [r for r in (0, grid - 1, grid, B - 1) if r < B]
    with SV(n) as sv:
        sv.set_option("force_path", 1)
        P.install(sv)
        for H in standard_hams(rng, n):
            sv.set_hamiltonian(H.op)
            e = sv.energy_batch(thetas)
            f = assert_launch(sv, n, real, B, K)
            assert f["workgroups"] == min(B, grid)
            if B > grid:
                assert f["workgroups"] < B     # some workgroup takes a second evaluation
                # the second (third) trip of a workgroup: same theta, same instructions, on a state and a table that were used before
                assert np.array_equal(e[grid:], e[:B - grid])
            check_rows(e, rows, thetas, P.state, H, (n, real, B))


@pytest.mark.parametrize("B", [1024, 1025, 2 * 1024 + 3])
@pytest.mark.parametrize("real", [False, True], ids=["complex", "real"])
@pytest.mark.parametrize("n", [5, 11])
def test_batch_wraps_the_grid_state_in_lds(SV, n, real, B):
    """1024 workgroups at most with the state in LDS: evaluation b + 1024 re-initialises |hf> over evaluation b's state and
    restages the cos/sin table"""
    assert lds_state(n, real)
    _wrap_case(SV, n, real, B, 1024)


@pytest.mark.parametrize("B", [512, 513, 1027])
@pytest.mark.parametrize("n,real", [(14, False), (15, True), (15, False)], ids=["14-complex", "15-real", "15-complex"])
def test_batch_wraps_the_grid_state_in_a_global_slice(SV, n, real, B):
    """512 workgroups at most with the state in a global slice per workgroup: evaluation b + 512 reuses the slice of b"""
    assert not lds_state(n, real)
    _wrap_case(SV, n, real, B, 512)


# ------------------------------------------------------------------------------------------------------ instance switches
INSTANCE_CASES = [(n, False, 1) for n in (1, 2, 8, 9, 10, 11, 13, 14, 15, 16)] + \
                 [(n, True, rm) for n in (14, 15) for rm in (1, 0)]


@pytest.mark.parametrize("n,real_program,real_mode", INSTANCE_CASES)
def test_instance_switches(SV, n, real_program, real_mode):
    """thread counts 64 -> 256 at n = 8/9 and 256 -> 1024 at 10/11, LDS -> global slice at 13/14 (complex) and 14/15 (real), from
    |0..0> and from |1..1>; a program that qualifies for real amplitudes runs complex with real_mode = 0"""
    rng = np.random.default_rng(2000 + 10 * n + 2 * real_program + real_mode)
    K = 3
    real = bool(real_program and real_mode)
    base = rng.uniform(-1, 1, (3, K))
    hams = standard_hams(rng, n)
    for hf in (0, (1 << n) - 1):
        P = dense_program(rng, n, real_program, K, hf)
        assert P.is_real() == real_program
        with SV(n) as sv:
            sv.set_option("force_path", 1)
            sv.set_option("real_mode", real_mode)
            P.install(sv)
            for B in ((1, 33) if n >= 15 else (3,)):
                thetas = base[np.arange(B) % 3]
                for H in hams:
                    sv.set_hamiltonian(H.op)
                    e = sv.energy_batch(thetas)
                    assert_launch(sv, n, real, B, K)
                    check_rows(e, list(range(min(B, 3))) + [B - 1], thetas, P.state, H, (n, hf, B))
                    if B > 3:
                        assert np.array_equal(e[3:], e[np.arange(3, B) % 3])


# -------------------------------------------------------------------------------------------------------------- table ops
def _uccsd_rotations(n):
    """UCCSD generators (2 occupied spatial orbitals) on the first 2 * (n // 2) qubits of an n-qubit register, thinned: singles and
    doubles; at n = 15 also one excitation whose x mask holds index bit 14 and one whose z mask outside x holds it
    -> [(xs, zs, coeffs)] per generator"""
    from openvqe_amd import fermion
    from openvqe_amd.backend import compile_ucc_program
    gens = fermion.uccsd_generators(n // 2, 2)
    gens = gens[:: max(1, len(gens) // 10)]
    xs, zs, cs, ps, K = compile_ucc_program(n, gens)
    out = [([int(x) for x in xs[ps == k]], [int(z) for z in zs[ps == k]], [float(c) for c in cs[ps == k]]) for k in range(K)]
    if n == 15:
        out.append(pattern_excitation([14], [5], chain=range(6, 14)))          # x mask with bit 14 (qubit 0 is occupied)
        out.append(pattern_excitation([12], [3], chain=[13, 14]))              # z outside x with bit 14
        out.append(pattern_excitation([14, 11], [9, 2], chain=[13, 12, 8, 7, 6, 5, 4, 3]))
        assert out[-3][0][0] >> 14 and not out[-2][0][0] >> 14 and (out[-2][1][0] & ~out[-2][0][0]) >> 14
    return out


def _sector_ham(rng, n, gens):
    """terms that see a particle-conserving state: per excitation two hopping strings on its x mask (even #Y, its own outside z
    mask) and random diagonal strings"""
    xs, zs = [], []
    for gx, gz, _ in gens:
        x = gx[0]
        zc = gz[0] & ~x
        bits = [b for b in range(n) if (x >> b) & 1]
        xs += [x, x]
        zs += [zc, zc | (1 << bits[0]) | (1 << bits[-1])]
    for _ in range(12):
        xs.append(0)
        zs.append(int(rng.integers(1, 1 << n)))
    keep = sorted(set(zip(xs, zs)))
    return MaskHam(n, [k[0] for k in keep], [k[1] for k in keep], rng.normal(size=len(keep)), 0.25)


@pytest.mark.parametrize("start", ["hf", "dense"])
@pytest.mark.parametrize("n", [12, 14, 15, 16])
def test_table_ops_streams_and_in_kernel_indices(SV, n, start):
    """commuting-run table ops through the host-built index stream (index_streams = 1; n <= 15: bit 14 of the index next to the sign
    bit 15 of the 16-bit word) and through in-kernel indices with the zero-pair skip (0; at n = 16 always), on real and on complex
    amplitudes; from the Hartree-Fock determinant, where the skip fires on most pairs, and behind a dense layer, where it never does"""
    from openvqe_amd import fermion
    rng = np.random.default_rng(3000 + n + (start == "dense"))
    gens = _uccsd_rotations(n)
    G = len(gens)
    K = G + (n if start == "dense" else 0)
    P = Prog(n, fermion.hf_integer(n, 4), K)
    if start == "dense":
        for b in range(n):
            P.add(1 << b, 1 << b, 1.0, G + b)
    for k, (gx, gz, gc) in enumerate(gens):
        for x, z, c in zip(gx, gz, gc):
            P.add(x, z, c, k)
    assert P.is_real()
    thetas = rng.uniform(-0.6, 0.6, (2, K))
    hams = standard_hams(rng, n) + [_sector_ham(rng, n, gens)]
    out = {}
    with SV(n) as sv:
        sv.set_option("force_path", 1)
        P.install(sv)
        info = sv.program_info()
        assert info["fused_ops"] < info["rotations"]       # the runs became table ops
        for real_mode in (1, 0):
            sv.set_option("real_mode", real_mode)
            for streams in (1, 0):
                sv.set_option("index_streams", streams)
                for h, H in enumerate(hams):
                    sv.set_hamiltonian(H.op)
                    e = sv.energy_batch(thetas)
                    assert_launch(sv, n, bool(real_mode), 2, K)
                    check_rows(e, (0, 1), thetas, P.state, H, (n, start, real_mode, streams, h))
                    out[real_mode, streams, h] = e
    psi = P.state(thetas[0])
    if start == "dense":
        assert np.count_nonzero(psi) == 1 << n
    else:
        assert np.count_nonzero(np.abs(psi) > 1e-14) < (1 << n) // 8
    for real_mode in (1, 0):
        for h, H in enumerate(hams):
            # the two index forms rotate the same pairs by the same angles
            assert np.abs(out[real_mode, 1, h] - out[real_mode, 0, h]).max() < TOL * H.scale


# --------------------------------------------------------------------------------------------------------------- segments
def _run_program_case(SV, P, rng, want_segments, B=2, real=False):
    entries = split_runs(P.runs())
    assert expected_segments(entries) == want_segments
    thetas = rng.uniform(-1, 1, (B, P.K))
    with SV(P.n) as sv:
        sv.set_option("force_path", 1)
        P.install(sv)
        assert sv.program_info()["fused_ops"] == len(entries)      # no run became a table op: the model above is the program
        for H in standard_hams(rng, P.n):
            sv.set_hamiltonian(H.op)
            e = sv.energy_batch(thetas)
            f = assert_launch(sv, P.n, real, B, P.K)
            assert f["segments"] == want_segments, f
            check_rows(e, range(B), thetas, P.state, H)
            if B > 1 and P.K == 0:
                assert np.array_equal(e, np.full(B, e[0]))


@pytest.mark.parametrize("R,diag,segments", [(511, False, 2), (512, False, 2), (513, False, 3), (1025, False, 4), (513, True, 3),
                                             (1025, True, 4)])
@pytest.mark.parametrize("n", [4, 11])
def test_one_run_longer_than_the_table(SV, n, R, diag, segments):
    """one same-x run of R rotations with independent parameters (no table op) behind the dense layer: split into ops of 512
    entries, each its own segment behind the layer's; diag: an x = 0 run, whose pieces straddle the segment boundaries"""
    rng = np.random.default_rng(4000 + n + R + diag)
    K = 5
    P = Prog(n, int(rng.integers(0, 1 << n)), K)
    dense_layer(P, rng, False, list(range(K)), phi0=True)
    x = 0 if diag else int(rng.integers(1, 1 << n)) | 2
    assert x != P.rx[-1]
    for r in range(R):
        P.add(x, int(rng.integers(1, 1 << n)), rng.uniform(-0.3, 0.3), r % K, rng.uniform(-0.2, 0.2) if r % 3 == 0 else 0.0)
    assert P.runs()[-1] == R
    _run_program_case(SV, P, rng, segments)


@pytest.mark.parametrize("second,segments", [(212, 1), (213, 2)])
@pytest.mark.parametrize("n", [4, 11])
def test_table_entries_cross_512_between_two_ops(SV, n, second, segments):
    """layer + run of 300 entries in all, then a run of 212 (the table is exactly full: one segment) or 213 (a second one)"""
    rng = np.random.default_rng(4100 + n + second)
    K = 5
    P = Prog(n, int(rng.integers(0, 1 << n)), K)
    dense_layer(P, rng, False, list(range(K)), phi0=True)
    xa = (1 << (n - 1)) | 1
    xb = (1 << (n - 1)) | 2
    for x, count in ((xa, 300 - 2 * n), (xb, second)):
        for r in range(count):
            P.add(x, int(rng.integers(0, 1 << n)), rng.uniform(-0.3, 0.3), r % K, rng.uniform(-0.2, 0.2) if r % 3 == 0 else 0.0)
    assert sum(P.runs()) == 300 + second and P.runs()[-2:] == [300 - 2 * n, second]
    _run_program_case(SV, P, rng, segments)


def _gate_oracle(n, hf, gates, theta):
    psi = np.zeros(1 << n, np.complex128)
    psi[hf] = 1.0
    for name, qs, sc, co, p in gates:
        if name == "CNOT":
            psi = masks.gate_cnot(psi, n, qs[0], qs[1])
        else:
            ang = co + (sc * theta[p] if p >= 0 else 0.0)
            psi = masks.gate_1q(psi, n, qs[0], dense.gate_matrix(name, ang))
    return psi


@pytest.mark.parametrize("T,segments", [(191, 1), (192, 1), (193, 2), (385, 3)])
@pytest.mark.parametrize("real", [False, True], ids=["complex", "real"])
@pytest.mark.parametrize("n", [4, 11])
def test_gate_programs_around_192_ops(SV, n, real, T, segments):
    """literal gate programs of T ops: H on every qubit, six rotation gates, a stretch of X / H / CNOT gates, and — except at
    T = 193, whose op 192 is then a segment of one literal gate — a last rotation gate.  At T = 385 ops 192..383 are literal
    gates: a segment without table entries (rot0 = rot1 = 0) between two that have some"""
    rng = np.random.default_rng(4200 + n + T + real)
    K = 3
    gates = [("H", [q], 0.0, 0.0, -1) for q in range(n)]
    names = ["RY"] * 6 if real else ["RY", "RZ", "RX", "RY", "RZ", "RX"]
    for g, name in enumerate(names):   # neighbouring rotation gates on different qubits: no two share a sweep
        gates.append((name, [g % n], float(rng.choice([1.0, -1.0, -2.0])), 0.0 if g % 2 == 0 else float(rng.uniform(-1, 1)), g % K))
    tail = 0 if T == 193 else 1
    for _ in range(T - n - 6 - tail):
        name = str(rng.choice(["X", "H", "CNOT"]))
        if name == "CNOT":
            c, t = rng.choice(n, 2, replace=False).tolist()
            gates.append((name, [c, t], 0.0, 0.0, -1))
        else:
            gates.append((name, [int(rng.integers(0, n))], 0.0, 0.0, -1))
    if tail:
        gates.append(("RY" if real else "RX", [n - 1], 1.0, 0.3, 1))
    assert len(gates) == T
    entries = [0 if g[0] in ("X", "H", "CNOT") else 1 for g in gates]
    assert expected_segments(entries) == segments
    if T == 385:
        assert sum(entries[192:384]) == 0 and entries[384] == 1
    hf = int(rng.integers(0, 1 << n))
    thetas = rng.uniform(-1, 1, (2, K))
    cache = {}

    def state(theta):
        key = theta.tobytes()
        if key not in cache:
            cache[key] = _gate_oracle(n, hf, gates, theta)
        return cache[key]

    with SV(n) as sv:
        sv.set_option("force_path", 1)
        sv.set_option("clifford_frame", 0)      # the literal list, gate by gate
        sv.set_gate_program(gates, K, hf)
        assert sv.program_info()["fused_ops"] == T
        for H in standard_hams(rng, n):
            sv.set_hamiltonian(H.op)
            e = sv.energy_batch(thetas)
            f = assert_launch(sv, n, real, 2, K)
            assert f["segments"] == segments, f
            check_rows(e, (0, 1), thetas, state, H, (n, real, T))


@pytest.mark.parametrize("real", [False, True], ids=["complex", "real"])
def test_constant_angles_only(SV, real):
    """K = 0: every angle is a phi0, B = 3 evaluations of the same circuit"""
    n = 5
    rng = np.random.default_rng(4300 + real)
    P = Prog(n, 0b10110, 0)
    dense_layer(P, rng, real, [])
    entanglers(P, rng, real, 5, [])
    assert P.is_real() == real and all(p < 0 for p in P.rp)
    _run_program_case(SV, P, rng, 1, B=3, real=real)


def test_constant_part_beside_a_parameter(SV):
    """phi = c * theta[p] + phi0 with both parts non-zero on every rotation"""
    n = 5
    rng = np.random.default_rng(4400)
    P = Prog(n, 0b00101, 2)
    dense_layer(P, rng, False, [0, 1], phi0=True)
    for _ in range(8):
        P.add(int(rng.integers(0, 1 << n)), int(rng.integers(1, 1 << n)), rng.uniform(-1, 1), int(rng.integers(0, 2)),
              rng.uniform(0.1, 0.7))
    assert all(p >= 0 and f != 0.0 for p, f in zip(P.rp, P.phi0))
    _run_program_case(SV, P, rng, 1)


# ------------------------------------------------------------------------------------------------------ expectation forms
_FIXED = {}


def fixed_state_program(n, real):
    """one dense state per (n, amplitude mode) for the expectation cases: program, parameter row"""
    if (n, real) not in _FIXED:
        rng = np.random.default_rng(5000 + 2 * n + real)
        P = dense_program(rng, n, real, 3, hf=int(rng.integers(0, 1 << n)), n_ent=4)
        _FIXED[n, real] = (P, rng.uniform(-1, 1, (1, 3)))
    return _FIXED[n, real]


def _expectation_case(SV, n, real, H, entries=None, flat=None, chunks=None, force_paths=(1,)):
    P, thetas = fixed_state_program(n, real)
    with SV(n) as sv:
        P.install(sv)
        for fp in force_paths:
            sv.set_option("force_path", fp)
            for k, Hk in enumerate((H, z_sum(n), wide_x(n))):      # the case, then two readings of the same state
                sv.set_hamiltonian(Hk.op)
                e = sv.energy_batch(thetas)
                f = assert_launch(sv, n, real, 1, 3)
                if fp != 1:
                    assert "declined" in sv.sparse_forms()      # no compact support: the default path falls to the fused kernel
                if k == 0:
                    if entries is not None:
                        assert f["exp_entries"] == entries, f
                    if flat is not None:
                        assert f["flat_items"] == flat, f
                    if chunks is not None:
                        assert f["exp_chunks"] == chunks, f
                check_rows(e, (0,), thetas, P.state, Hk, (n, real, k, fp))


def deposit(m, x, n):
    """the bits of m on the index positions outside x, ascending"""
    out, k = 0, 0
    for b in range(n):
        if not (x >> b) & 1:
            out |= ((m >> k) & 1) << b
            k += 1
    return out


def _distinct_masks(rng, count, nbits, must=()):
    out = list(dict.fromkeys(int(m) for m in must))
    seen = set(out)
    while len(out) < count:
        m = int(rng.integers(1, 1 << nbits))
        if m not in seen:
            seen.add(m)
            out.append(m)
    return out[:count]


@pytest.mark.parametrize("n", [6, 7, 8, 9, 10, 11, 12, 13, 14])
def test_diagonal_group_alone(SV, n):
    """2^n free indices against the thread count: the direct loop (n = 6), M = 2 / 4 WHT points under 64 (7, 8), 256 (9, 10) and
    1024 threads (11, 12), M = 8 (13) and M = 8 with two trips on a state in a global slice (14); masks with each single index
    bit, so every bucket bit above the thread bits is set by some term"""
    rng = np.random.default_rng(5100 + n)
    zs = _distinct_masks(rng, 40, n, must=[1 << b for b in range(n)] + [(1 << n) - 1])
    H = MaskHam(n, [0] * len(zs), zs, rng.normal(size=len(zs)), 0.5)
    _expectation_case(SV, n, False, H, entries=1, flat=0, chunks=1)


@pytest.mark.parametrize("w", [1, 2, 4, 7, 8])
@pytest.mark.parametrize("n", [10, 13])
def test_group_widths(SV, n, w):
    """one x-group of width w: 2^(w-1) (group, pattern) entries up to w = 7, the dense form (pivot only) at w = 8; the x mask
    stays below the three highest index bits, which then are the highest free-index bits — the bucket bits — and terms set each
    of them alone and together"""
    rng = np.random.default_rng(5200 + 10 * n + w)
    xbits = sorted(rng.choice(n - 3 if w <= n - 3 else n - 2, w, replace=False).tolist())   # (n = 10, w = 8: bits 0..7)
    x = sum(1 << b for b in xbits)
    top = [1 << (n - 1), 1 << (n - 2), 1 << (n - 3)]
    zs = _distinct_masks(rng, 24, n, must=top + [top[0] | top[1] | top[2], top[0] | x, top[1] | (x & -x)])
    H = MaskHam(n, [x] * len(zs), zs, rng.normal(size=len(zs)), -0.25)
    entries = (1 << (w - 1)) if w <= 7 else 1
    merged = len({z & ~x for z in zs}) if w <= 7 else len(zs)     # terms of an entry: one per distinct mask outside x
    assert 2 <= merged <= STAGE_CAP
    per_chunk = STAGE_CAP // merged                               # whole entries that fit the staging area
    _expectation_case(SV, n, False, H, entries=entries, flat=0, chunks=-(-entries // per_chunk))


@pytest.mark.parametrize("n,w,flat", [(6, 1, 1), (7, 1, 4), (8, 3, 4), (9, 3, 16)])
def test_single_real_term_groups(SV, n, w, flat):
    """one real-coefficient term per x-group: entry-per-lane flat items, one per pattern with 2^(n-w) = 32 free indices, four
    slices each with 64; w = 3 has four patterns.  Two such groups, so lanes hold different items"""
    rng = np.random.default_rng(5300 + 10 * n + w)
    xs, zs = [], []
    for g in range(2):
        xbits = sorted(rng.choice(n, w, replace=False).tolist())
        x = sum(1 << b for b in xbits)
        while x in xs:
            xbits = sorted(rng.choice(n, w, replace=False).tolist())
            x = sum(1 << b for b in xbits)
        z = int(rng.integers(1, 1 << n)) & ~x
        if w == 3 and g == 0:
            z |= (1 << xbits[0]) | (1 << xbits[2])       # two Y: still a real coefficient
        xs.append(x)
        zs.append(z)
    H = MaskHam(n, xs, zs, rng.normal(size=2), 0.0)
    _expectation_case(SV, n, False, H, entries=0, flat=2 * flat, chunks=0)


def test_real_mode_drops_odd_y_terms(SV):
    """real amplitudes: a group whose terms all have an odd number of Y leaves no entry; a group with even and odd ones keeps the
    even ones (the oracle evaluates all of them: the odd ones vanish on the real state)"""
    n = 9
    rng = np.random.default_rng(5400)
    xa, xb = 0b000110100, 0b101000010
    xs, zs = [], []
    for _ in range(6):
        z = int(rng.integers(0, 1 << n))
        if not bin(xa & z).count("1") & 1:
            z ^= xa & -xa
        xs.append(xa)
        zs.append(z)
    # distinct masks outside xb: nothing merges, so every pattern keeps as many terms as have an even number of Y
    zb = [deposit(m, xb, n) | (int(rng.integers(0, 1 << n)) & xb) for m in _distinct_masks(rng, 12, n - 3)]
    assert 2 <= sum(1 for z in zb if not bin(xb & z).count("1") & 1) <= 10
    xs += [xb] * len(zb)
    zs += zb
    keep = sorted(set(zip(xs, zs)))
    H = MaskHam(n, [k[0] for k in keep], [k[1] for k in keep], rng.normal(size=len(keep)), 0.0)
    P, thetas = fixed_state_program(n, True)
    assert np.abs(P.state(thetas[0]).imag).max() < 1e-15
    _expectation_case(SV, n, True, H, entries=4, flat=0, chunks=1)      # xb: w = 3, four patterns; xa: nothing


@pytest.mark.parametrize("second,chunks", [(341, 1), (342, 2)])
def test_term_staging_chunks(SV, second, chunks):
    """two w = 1 groups of 341 + 341 = 682 merged terms fill the staging area exactly; 341 + 342 need a second chunk"""
    n = 10
    rng = np.random.default_rng(5500 + second)
    xs, zs = [], []
    for x, count in ((1 << 3, 341), (1 << 7, second)):
        for m in _distinct_masks(rng, count, n - 1):       # distinct masks on the other nine bits: nothing merges
            xs.append(x)
            zs.append(deposit(m, x, n))
    assert 341 + second == (STAGE_CAP if chunks == 1 else STAGE_CAP + 1)
    H = MaskHam(n, xs, zs, rng.normal(size=len(xs)), 0.0)
    _expectation_case(SV, n, False, H, entries=2, flat=0, chunks=chunks)


# -------------------------------------------------------------------------------------------------------- oversized groups
def _oversized(kind):
    rng = np.random.default_rng(5600)
    if kind == "all_z_strings_10":
        n = 10
        zs = list(range(1, 1 << n))
        return n, MaskHam(n, [0] * len(zs), zs, rng.normal(size=len(zs)), 0.0), 2
    if kind == "w1_1024_outside_masks_11":
        n = 11
        x = 1 << 4
        zs = [deposit(m, x, n) for m in range(1 << (n - 1))]
        return n, MaskHam(n, [x] * len(zs), zs, rng.normal(size=len(zs)), 0.0), 2
    n = 10
    x = 0b0111101111
    zs = _distinct_masks(rng, 700, n)
    return n, MaskHam(n, [x] * len(zs), zs, rng.normal(size=len(zs)), 0.0), 2


@pytest.mark.parametrize("kind", ["all_z_strings_10", "w1_1024_outside_masks_11", "w8_700_terms_10"])
def test_groups_longer_than_the_staging_area(SV, kind):
    """one emitted term list longer than the 682 terms the staging area holds is evaluated in consecutive entries with the same
    pairs, on the default path (the program has no compact support) and under force_path = 1"""
    n, H, entries = _oversized(kind)
    assert len(H.cs) > STAGE_CAP
    _expectation_case(SV, n, False, H, entries=entries, flat=0, chunks=entries, force_paths=(0, 1))


# --------------------------------------------------------------------------------------------------------------- I/O forms
def test_io_forms_agree_bit_for_bit(SV):
    """the same kernel behind the polled mapped buffer (B <= 256), the mapped buffer (B <= 1024 and B (K + 1) <= 131072 doubles),
    staged copies, and the device-resident entry: one parameter table, cycled; the same theta gives the same bits everywhere"""
    import torch
    n, P_ROWS, K_USED = 6, 64, 127
    rng = np.random.default_rng(6000)
    hams = standard_hams(rng, n)
    table = rng.uniform(-1, 1, (P_ROWS, 128))
    ref = None
    seen = set()
    for K, B in ((127, 256), (127, 257), (127, 1024), (127, 1025), (128, 1016), (128, 1017)):
        prng = np.random.default_rng(6001)         # the same rotations for both K: parameter 127 is declared, not used
        P = Prog(n, 0b011010, K)
        dense_layer(P, prng, False, list(range(K_USED)))
        for p in range(K_USED):
            P.add(int(prng.integers(0, 1 << n)), int(prng.integers(1, 1 << n)), prng.uniform(-0.5, 0.5), p, prng.uniform(-0.2, 0.2))
        thetas = np.ascontiguousarray(table[np.arange(B) % P_ROWS, :K])
        td = torch.from_numpy(thetas).cuda()
        with SV(n) as sv:
            sv.set_option("force_path", 1)
            P.install(sv)
            got = []
            for H in hams:
                sv.set_hamiltonian(H.op)
                e = sv.energy_batch(thetas)
                assert_launch(sv, n, False, B, K)
                seen.add(io_form(B, K))
                ed = torch.zeros(B, dtype=torch.float64, device="cuda")
                sv.energy_batch_device(B, td.data_ptr(), ed.data_ptr())
                assert_launch(sv, n, False, B, K, device=True)
                assert np.array_equal(ed.cpu().numpy(), e)
                check_rows(e, (0, P_ROWS - 1, B - 1), thetas, P.state, H, (K, B))
                got.append(e)
            if ref is None:
                ref = [e[:P_ROWS].copy() for e in got]
                # the mapped buffer without polling: a stream synchronisation instead
                sv.set_option("poll_result", 0)
                e8 = sv.energy_batch(thetas[:8])
                assert_launch(sv, n, False, 8, K, poll=False)
                assert np.array_equal(e8, ref[-1][:8])
                sv.set_option("poll_result", 1)
            for h in range(len(hams)):
                assert np.array_equal(got[h], ref[h][np.arange(B) % P_ROWS]), (K, B, h)
    assert 1024 * (127 + 1) == IO_DOUBLES and 1016 * 129 <= IO_DOUBLES < 1017 * 129
    assert seen == {"polled", "mapped", "staged"}
