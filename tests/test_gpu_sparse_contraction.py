"""The contraction of k_sparse_vqe_rows_shared (sv_sparse.hpp) reads one slot group ahead: the pieces of a thread are ONE sequence
of RPT (EPR + 1) read groups, group g + 1 in flight while group g is consumed.  What such a loop can get wrong sits at the ends of
the sequence and at the piece boundaries, so the restricted Hamiltonians here are designed for them, on designed supports
(tests/util.py: cascade_geometry) that take the LiH instance (RPT 1, EPR 17: supports up to 256 states) and the H2O instance
(RPT 4, EPR 10: a support of 384 states):

  diagonal    Z strings only: every entry is (i, i), every piece holds ONE real slot — its owner — and EPR - 1 of padding
  one_string  one off-diagonal string on the x mask of the program's first rotation, plus the constant: a few pieces of one entry,
              almost every slot zero padding, the last groups of every thread all padding
  full        random strings, one x mask each, added until the next one would make the instance decline: pieces filled to their
              last slot (128 states on the LiH instance: 256 pieces on 256 threads, every row one piece of 17 real slots and one
              more), the last slot of the last piece a real coefficient
  split_row   more than EPR entries per state on average: rows split over several pieces (more pieces than states)
  no_entry    no entry on the support at all.  The workgroup geometry declines a program without entries (launch_rows_shared:
              nent >= 1), so this case names the geometry that runs instead, "per_wave"; the energies are the constant exactly.

Every case runs batches of 2048 + 3 and 2048 + 5 evaluations (the last work item of 8 is partial), asserts the geometry that ran
and, from program_info, the shape it reached, compares with the C oracle on _sample_shared(B) within 1e-11 x max(1, |H|_1) — the
bound of the sparse tests — and asks for identical bits from two launches."""
import numpy as np
import pytest

from openvqe_amd.operators import Hamiltonian
from tests.test_gpu_sparse import Case, _designed, _mask_term, _thetas_with_nan_tail
from tests.test_gpu_sparse_shared import H2O_GEOMETRY, LIH_GEOMETRY, T, _device_batch, _sample_shared
from tests.util import cascade_geometry, support_closure

pytestmark = pytest.mark.gpu

NT = 256
# sparse_host.inc, SHARED_13 / SHARED_37: geometry -> (pieces per thread, slots per piece, entries per thread of the criterion)
SHAPE = {LIH_GEOMETRY: (1, 17, 13), H2O_GEOMETRY: (4, 10, 37)}
# cascade_geometry(k, t, d): 64, 128 and 256 states closed under every x mask on bits 1 .. k; 255 = every state of 8 bits but 0;
# 384 = 256 states with bit 0 set + 128 with bit 0 clear and bit 1 set
SUPPORTS = {64: (6, 0, 0), 128: (7, 0, 0), 255: (7, 7, 0), 256: (8, 0, 0), 384: (8, 1, 0)}
BATCHES = (T + 3, T + 5)


def _program(m):
    """the designed program of m basis states -> (a Case with the helper's Hamiltonian, the support as a set)"""
    n, hf, gens, K = cascade_geometry(*SUPPORTS[m])
    base = _designed(n, hf, gens, K, seed=m)
    S = support_closure(base.hf, base.rx, base.rz, base.rc, base.rp)
    assert S.size == m
    return base, set(int(a) for a in S)


def _string(rng, n, x):
    """a real string on the x mask x: an even number of Y inside x, random Z outside"""
    bits = [b for b in range(n) if (x >> b) & 1]
    ys = [b for b in bits if rng.random() < 0.5]
    if len(ys) % 2:
        ys = ys[1:]
    z = sum(1 << b for b in ys) | (int(rng.integers(0, 1 << n)) & ~x)
    if x == 0 and z == 0:
        z = 1
    return x, z, float(rng.normal())


def _z_strings(rng, n, count):
    seen, out = set(), []
    while len(out) < count:
        x, z, c = _string(rng, n, 0)
        if z not in seen:
            seen.add(z)
            out.append((0, z, c))
    return out


def _x_masks(rng, n, S, count):
    """count distinct x masks (random order) that connect at least one pair of the support"""
    masks = [x for x in range(1, 1 << n) if any((a ^ x) in S for a in S)]
    assert len(masks) >= count, (len(masks), count)
    return [masks[i] for i in rng.permutation(len(masks))[:count]]


def _with(base, strings, constant):
    H = Hamiltonian(base.n, [_mask_term(base.n, x, z, c) for x, z, c in strings], float(constant))
    return Case(base.n, base.hf, base.rx, base.rz, base.rc, base.rp, base.K, H)


def _entries(S, strings):
    """entries of the restricted Hamiltonian: per distinct x mask the states (x = 0) or the unordered pairs of the support"""
    total = 0
    for x in set(x for x, _, _ in strings):
        total += len(S) if x == 0 else sum(1 for a in S if (a ^ x) in S) // 2
    return total


def _packed_slots(case):
    """slots per thread of the instance that packed the program (0: none did)"""
    from openvqe_amd.backend import Statevector
    with Statevector(case.n) as sv:
        sv.set_hamiltonian(case.H)
        case.program(sv)
        sv.energy_batch(np.zeros((2, case.K)))
        return sv.program_info()["sp_h_slots"]


def _build(m, kind):
    """-> (case, the geometry it must run on, entries the restricted Hamiltonian must have, extra assertions on program_info)"""
    base, S = _program(m)
    n = base.n
    rng = np.random.default_rng(1000 * m + len(kind))
    geometry = LIH_GEOMETRY if m <= 256 else H2O_GEOMETRY
    rpt, epr, ept = SHAPE[geometry]
    checks = []
    if kind == "diagonal":
        strings = _z_strings(rng, n, 12)
        checks.append(lambda info: info["sp_h_pieces"] == m)                      # one piece per state, one real slot in each
    elif kind == "one_string":
        x = int(base.rx[0])
        strings = [(x, 0, 0.75)]
        checks.append(lambda info: info["sp_h_pieces"] <= info["sp_h_entries"] <= m // 2)   # pieces of one or two entries: the rest is padding
    elif kind == "split_row":
        # closed supports: every x mask adds m / 2 entries; more than EPR entries per state
        count = {64: 40, 128: 40, 256: 30, 384: 40}[m]
        if m == 256:
            geometry = H2O_GEOMETRY   # 256 + 30 * 128 entries are beyond the LiH instance's 256 * 13: the H2O instance, rows of ~16 on pieces of 10
            rpt, epr, ept = SHAPE[geometry]
        strings = _z_strings(rng, n, 3) + [_string(rng, n, x) for x in _x_masks(rng, n, S, count)]
        checks.append(lambda info: info["sp_h_entries"] > epr * m)                # some state owns more than EPR entries ...
        checks.append(lambda info: info["sp_h_pieces"] > m)                       # ... and more than one piece
    elif kind == "full":
        pool = _z_strings(rng, n, 3) + [_string(rng, n, x) for x in _x_masks(rng, n, S, 96)]
        want = rpt * epr
        lo, hi = 4, len(pool)
        assert _packed_slots(_with(base, pool[:lo], 0.5)) == want
        assert _packed_slots(_with(base, pool[:hi], 0.5)) != want, "the pool of strings does not reach the instance's capacity"
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if _packed_slots(_with(base, pool[:mid], 0.5)) == want:
                lo = mid
            else:
                hi = mid
        strings = pool[:lo]   # the instance takes these; with pool[lo] added it declines
        checks.append(lambda info: info["sp_h_entries"] <= NT * ept and info["sp_h_pieces"] <= NT * rpt)
        checks.append(lambda info: info["sp_h_pieces"] > NT * rpt // 2)          # more than half of all pieces in use
    elif kind == "no_entry":
        strings = [(1, 0, 0.75), (1, 6, -0.5)]   # x = bit 0: every state of these supports has bit 0 set, no partner has
        geometry = "per_wave"
        checks.append(lambda info: info["sp_h_pieces"] == 0 and info["sp_h_slots"] == 0)
    else:
        raise AssertionError(kind)
    return _with(base, strings, 0.5), geometry, _entries(S, strings), checks


CASES = [(m, kind) for m in (64, 128, 255, 384) for kind in ("diagonal", "one_string")] + \
        [(128, "full"), (255, "full"), (384, "full")] + \
        [(64, "split_row"), (128, "split_row"), (256, "split_row"), (384, "split_row")] + \
        [(64, "no_entry"), (128, "no_entry")]


@pytest.mark.parametrize("m, kind", CASES, ids=[f"{kind}-{m}" for m, kind in CASES])
def test_contraction_at_the_ends_of_the_group_sequence(gpu_lib, m, kind):
    from openvqe_amd.backend import Statevector
    case, geometry, entries, checks = _build(m, kind)
    with Statevector(case.n) as sv:
        sv.set_hamiltonian(case.H)
        case.program(sv)
        for B in BATCHES:
            full = _thetas_with_nan_tail(np.random.default_rng(7 * m + B), B, case.K, extra=64)
            e1, kept1 = _device_batch(sv, full, B)
            e2, kept2 = _device_batch(sv, full, B)
            # the geometry that ran, and the shape it reached
            assert sv.sparse_forms() == {"rows2"}
            assert sv.sparse_geometries() == {geometry}
            info = sv.program_info()
            print(f"{kind}, {m} states, B = {B}: {geometry}, entries {info['sp_h_entries']}, pieces {info['sp_h_pieces']}, "
                  f"slots {info['sp_h_slots']}, reads per state {info['sp_h_reads_per_state']}")
            assert info["support"] == m
            assert info["sp_h_entries"] == entries
            if geometry in SHAPE:
                rpt, epr, _ = SHAPE[geometry]
                assert info["sp_h_slots"] == rpt * epr and info["sp_h_reads_per_state"] == rpt * (epr + 1)
                assert -(-entries // epr) <= info["sp_h_pieces"] <= NT * rpt
            for check in checks:
                assert check(info), info
            # the oracle, and the same bits twice
            assert kept1 and kept2
            assert np.isfinite(e1).all()
            idx = _sample_shared(B)
            err = np.abs(e1[idx] - case.oracle(full[idx])).max()
            print(f"    max |E - oracle| on {idx.size} samples = {err:.3e} (bound {1e-11 * case.scale:.3e})")
            assert err < 1e-11 * case.scale
            assert np.array_equal(e1.view(np.int64), e2.view(np.int64))
            if kind == "no_entry":
                assert np.array_equal(e1, np.full(B, case.const))
