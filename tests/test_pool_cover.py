"""The host-side planner of the ADAPT pool screen on the partitioned register (openvqe_amd/csrc/sv_pool_host.hpp: pool terms by rank
difference, (operator, local x) entries, greedy cover of the distinct x masks by (tile bit set, displacement) passes, staged chunks
within the term and entry caps, pieces of oversized operators, runs of equal slots) compiled with g++ alone under ASan + UBSan:
tests/cpu/pool_cover_check.cpp replays the plan of every rank the way k_tile_pool / k_tile_pool_real / k_pool_small index it and
compares every v_k with the term-by-term definition to 1e-12 max(1, |c_k|_1), complex and real flavour."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pool_cover_planner_under_asan_ubsan(tmp_path):
    src = os.path.join(ROOT, "tests", "cpu", "pool_cover_check.cpp")
    exe = str(tmp_path / "pool_cover_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-o", exe, src])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    for seed in ("7", "2025"):
        r = subprocess.run([exe, "150", seed], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "pool cover ok" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]


def test_pool_symbols_are_declared_everywhere():
    """the ovqe_xpool_* exports in the header, the cffi declarations and the ctypes signatures"""
    from openvqe_amd import _lib
    names = ["ovqe_xpool_" + s for s in ("create", "destroy", "partners", "info", "local", "remote", "finish")]
    header = open(os.path.join(ROOT, "include", "ovqe_sv.h")).read()
    cdef = open(os.path.join(ROOT, "include", "ovqe_sv.cdef.h")).read()
    for name in names:
        assert name + "(" in header and name + "(" in cdef and name in _lib.SIGNATURES
