"""CPU tests of the case builders of tests/stream_cases.py: the constants the cases are derived from against the sources that hold
them, the 16 | 17 pair under the checkers, the dense cases' properties, the restated cover rule against the host-only header
(openvqe_amd/csrc/sv_cover_host.hpp) replayed by tests/cpu/apply_cover_check.cpp under ASan + UBSan with g++ alone, and the row count of
a full set of deflation vectors."""
import os
import subprocess

import numpy as np
import pytest

from tests import deflation_cases as dc
from tests import gradbatch_cases as gc
from tests import spread_cases as sp
from tests import stream_cases as st

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DENSE = [(13, False), (14, True)] + [(n, real) for n in (17, 19, 20) for real in (True, False)]


def _source(name):
    return open(os.path.join(ROOT, "openvqe_amd", "csrc", name)).read()


def test_constants_are_the_sources():
    """every constant of tests/stream_cases.py where the library defines it; the derived sizes"""
    main = _source("ovqe_sv.hip")
    assert f"constexpr int DEFLATE_MAX = {st.DEFLATE_MAX};" in _source("sv_deflate.hpp")
    assert f"constexpr int DEFLATE_CHUNK = {st.DEFLATE_CHUNK};" in _source("sv_deflate.hpp")
    assert f"constexpr int HAM_TILE_LOW = {st.TILE_LOW};" in _source("sv_cover_host.hpp")
    assert f"int opt_apply_min_tiles = {st.APPLY_MIN_TILES};" in main
    assert f"(h->n_local >= 25 ? 12 : {st.TILE_BITS})" in main
    assert f"std::min<uint64_t>({st.REDUCE_BLOCKS}, std::max<uint64_t>(1, (namps + {st.REDUCE_THREADS - 1}) / {st.REDUCE_THREADS}))" in main
    def body_of(name, fun):
        text = _source(name)
        body = text[text.index(f"int {fun}("):]
        return body[:body.index("\n}\n")]
    # the single gradient has the gate itself; the four batched calls have it in the ONE decision they all ask
    for name, fun in (("sparse_host.inc", "run_sparse_gradient"), ("gradbatch_host.inc", "compact_batch_plan")):
        assert f"h->n_local > {st.COMPACT_MAX_QUBITS}" in body_of(name, fun), fun
    for name, fun in (("gradbatch_host.inc", "run_grad_batch"), ("deflate_host.inc", "run_vqd_batch"), ("spread_host.inc", "run_spread_batch"),
                      ("constrain_host.inc", "run_constrained_batch")):
        assert "compact_batch_plan(h, B, &A, &G, &ok)" in body_of(name, fun), fun
    assert (st.TILED_FROM, st.SECOND_TRIP_FROM) == (19, 20)
    assert [st.tiled_by_default(n) for n in (17, 18, 19, 20)] == [False, False, True, True]
    assert [st.trips(n) for n in (14, 17, 19, 20)] == [1, 1, 1, 2] and st.reduce_blocks(1 << 14) == 64
    assert [st.deflation_launches(1, J) for J in (1, 4, 5, 32)] == [3, 6, 9, 48]


@pytest.mark.parametrize("leak", [True, False])
def test_boundary_pair(leak):
    """one program, term for term the same Hamiltonian and BOUNDARY_C Z on index bit 16: the checkers give E17 = E16 + c, the same
    variance and equal gradients; the support is closed under the Hamiltonian exactly when the leak term is left out"""
    lo, hi = st.boundary_pair(leak)
    assert (lo.n, hi.n, lo.K, hi.K) == (16, 17, 9, 9) and lo.n == st.COMPACT_MAX_QUBITS
    for a, b in zip((lo.rx, lo.rz, lo.rc, lo.pidx), (hi.rx, hi.rz, hi.rc, hi.pidx)):
        assert np.array_equal(a, b)
    assert int(np.bitwise_or.reduce(lo.rx | lo.rz)) == 0x7f and st.is_real_program(lo.rx, lo.rz)
    T = len(lo.h[2])
    assert len(hi.h[2]) == T + 1 == (22 if leak else 21)
    for k in range(3):
        assert np.array_equal(lo.h[k], hi.h[k][:T])
    assert (int(hi.h[0][T]), int(hi.h[1][T]), float(hi.h[2][T])) == (0, 1 << 16, st.BOUNDARY_C) and lo.h[3] == hi.h[3]
    pool = {0} | {int(x) for x in lo.rx} | {int(x) ^ int(y) for x in lo.rx for y in lo.rx}
    own = slice(0, T - 1 if leak else T)
    assert {int(x) for x in lo.h[0][own]} <= pool and any((int(z) >> 15) & 1 for z in lo.h[1]) and not any(int(z) >> 16 for z in lo.h[1])
    for case in (lo, hi):
        assert sp.case_exactness(case)[:2] == (False, leak)
    theta = st.thetas(lo, 1, 3)[0]
    (e16, g16), (e17, g17) = lo.want(theta), hi.want(theta)
    print(f"leak {leak}: E16 {e16:.12f} E17 - E16 - c {e17 - e16 - st.BOUNDARY_C:.3e} max |dg| {np.abs(g17 - g16).max():.3e}")
    assert abs(e17 - e16 - st.BOUNDARY_C) <= 1e-13 * hi.h1 and np.abs(g17 - g16).max() <= 1e-13 * hi.h1 and np.abs(g16).max() > 1e-2
    if not leak:
        (_, sg16, _, s16), (_, sg17, _, s17) = sp.case_want(lo, theta), sp.case_want(hi, theta)
        assert abs(s17 - s16) <= 1e-13 * hi.h1 ** 2 and np.abs(sg17 - sg16).max() <= 1e-13 * hi.h1 ** 2 and s16 > 1e-2


@pytest.mark.parametrize("n, real", DENSE)
def test_dense_cases(n, real):
    """n + 4 rotations, K = 24, 16 to 24 real terms; the complex program has no real form, reaches the top index bit and straddles the
    tile edge; the cover of the Hamiltonian at tiles of 2^11: at least two sweeps, every group in one of them, none left untiled"""
    case = st.dense(n, real)
    assert case is st.dense(n, real) and (case.n, case.K, len(case.rc)) == (n, gc.Y_K, n + 4) and n + 4 <= gc.Y_K
    assert st.is_real_program(case.rx, case.rz) == real and 16 <= len(case.h[2]) <= 24
    assert int(np.bitwise_or.reduce(case.rx)) == (1 << n) - 1            # every bit is rotated: the state fills the register
    assert all(int(a) != int(b) for a, b in zip(case.rx[:-1], case.rx[1:]))
    if real:
        base = gc.y_program(n + 4, n=n)
        assert all(np.array_equal(a, b) for a, b in zip((case.rx, case.rz, case.rc, case.pidx), (base.rx, base.rz, base.rc, base.pidx)))
    else:
        kinds = {(int(x) != 0, bin(int(x) & int(z)).count("1")) for x, z in zip(case.rx, case.rz)}
        assert kinds == {(True, 1), (True, 0), (True, 2), (False, 0)}       # odd Y, X-type, even Y, Z only
        assert any((int(x) >> (n - 1)) & 1 for x in case.rx)
        assert any((int(x) >> 10) & 3 == 3 for x in case.rx)               # a pair of a 2^11 tile with its neighbour
    assert all(bin(int(x) & int(z)).count("1") % 2 == 0 for x, z in zip(case.h[0], case.h[1]))   # a real-symmetric sum
    sweeps, rest = st.apply_cover(n, case.h[0])
    print(f"dense({n}, {real}): {len(case.h[2])} terms, {len(set(case.h[0].tolist()))} x-groups, sweeps {[hex(s) for s in sweeps]}, rest {rest}")
    assert len(sweeps) >= 2 and rest == 0
    assert all(bin(s).count("1") == st.TILE_BITS and s & 3 == 3 and s < (1 << n) for s in sweeps)
    assert all(any(not int(x) & ~s for s in sweeps) for x in case.h[0])


@pytest.fixture(scope="module")
def check_program(tmp_path_factory):
    src = os.path.join(ROOT, "tests", "cpu", "apply_cover_check.cpp")
    exe = str(tmp_path_factory.mktemp("cover") / "apply_cover_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-o", exe, src])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")

    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
        return r.stdout

    return run


def test_restated_cover_against_the_header(check_program, tmp_path):
    """``stream_cases.apply_cover`` against grow_tile_set of sv_cover_host.hpp: the cases of this file, the 16 | 17 pair, and random
    mask sets — wide masks that stay untiled, more groups than one set holds, tiles of 2^10 to 2^12"""
    cases = [(n, st.TILE_BITS, st.TILE_LOW, sorted(set(st.dense(n, real).h[0].tolist()))) for n, real in DENSE]
    cases += [(c.n, st.TILE_BITS, st.TILE_LOW, sorted(set(c.h[0].tolist()))) for c in st.boundary_pair()]
    rng = np.random.default_rng(11)
    for _ in range(120):
        M = int(rng.integers(10, 13))
        n, G = int(rng.integers(M + 2, 25)), int(rng.integers(3, 40))
        weight = int(rng.integers(1, 14))
        xs = {0, 1, 2} | {int(sum(1 << int(b) for b in rng.choice(n, size=int(rng.integers(1, weight + 1)), replace=False))) for _ in range(G)}
        cases.append((n, M, int(rng.integers(0, 5)), sorted(xs)))
    listing = tmp_path / "cases.txt"
    listing.write_text("".join(f"{n} {M} {low} {len(xs)} " + " ".join(str(x) for x in xs) + "\n" for n, M, low, xs in cases))
    out = check_program(listing)
    assert f"apply cover ok ({len(cases)} cases)" in out
    rows = [line.split() for line in out.splitlines() if line.startswith("case ")]
    assert len(rows) == len(cases)
    seen_rest = seen_many = False
    for row, (n, M, low, xs) in zip(rows, cases):
        sweeps, rest = st.apply_cover(n, xs, M, low)
        assert len(xs) >= 3 and n >= M + 2
        assert (int(row[1].split("=")[1]), int(row[2].split("=")[1]), [int(v) for v in row[3:]]) == (len(sweeps), rest, sweeps), (row, sweeps, rest)
        seen_rest, seen_many = seen_rest or rest > 0, seen_many or len(sweeps) >= 4
    assert seen_rest and seen_many


def test_untiled_registers_and_hamiltonians():
    """below TILE_BITS + 2 qubits, and with fewer than three x-groups, nothing is tiled: every group is rest"""
    assert st.apply_cover(12, [0, 1, 2, 4]) == ([], 4) and st.apply_cover(14, [0, 1 << 13]) == ([], 2)
    assert st.apply_cover(13, [0, 1, 1 << 12])[1] == 0


def test_vector_sets():
    """the sets of the GPU tests on ``gradbatch_cases.per_rotation(9)`` (7 qubits, the support is the whole register): compositions,
    distinct weights, and the real rows path 1 makes of them — a row per vector and one more per vector with an imaginary part: J = 32
    with thirty complex vectors, a real one and the real ansatz state gives 30 x 2 + 1 + 1 = 62 rows"""
    case = gc.per_rotation(9)
    want = {1: (1, 0, 0), 2: (1, 0, 1), 4: (1, 1, 2), 5: (1, 1, 3), 32: (30, 1, 1)}
    for J, (ncomplex, nreal, nansatz) in want.items():
        vset = st.vector_set(case, J, ncomplex=30 if J == 32 else 1)
        vectors = st.set_vectors(case, vset)
        assert len(vset) == J == ncomplex + nreal + nansatz and len({b for _, _, b in vset}) == J and all(b > 0 for _, _, b in vset)
        assert [k for k, _, _ in vset] == ["vector"] * (ncomplex + nreal) + ["ansatz"] * nansatz
        assert all(v.shape == (1 << case.n,) and abs(np.linalg.norm(v) - 1.0) <= 1e-12 for v in vectors)
        with_im = [bool(np.any(v.imag != 0.0)) for v in vectors]
        assert with_im == [True] * ncomplex + [False] * (nreal + nansatz)
        assert st.real_rows(vectors) == J + ncomplex == st.real_rows(vectors, np.arange(1 << case.n))
    assert st.real_rows(st.set_vectors(case, st.vector_set(case, 32, ncomplex=30))) == 62
    # the nested sets of the vector-count test: the same composition at J = 32, rows J + the complex vectors of every prefix
    nested = st.nested_set(case)
    vectors = st.set_vectors(case, nested)
    with_im = [bool(np.any(v.imag != 0.0)) for v in vectors]
    assert len(nested) == st.DEFLATE_MAX == 32 and len({b for _, _, b in nested}) == 32
    assert with_im == [True, False, False] + [True] * 29 and [k for k, _, _ in nested][:4] == ["vector", "vector", "ansatz", "vector"]
    assert [st.real_rows(vectors[:J]) for J in (1, 4, 5, 32)] == [2, 6, 8, 62] and 62 == 2 * 30 + 1 + 1
    # eight full passes of k_deflate_dots, no remainder; J = 5: a full pass and a remainder of one; J = 1: a remainder alone
    assert [(J // st.DEFLATE_CHUNK, J % st.DEFLATE_CHUNK) for J in (1, 4, 5, 32)] == [(0, 1), (1, 0), (1, 1), (8, 0)]
    assert dc.bound_overlap(vectors[0]) == pytest.approx(1e-12)
