"""The host-side planner of the cross-shard Pauli sums on the partitioned register (openvqe_amd/csrc/sv_cross_host.hpp over the shared
cover rule of sv_cover_host.hpp: groups by rank difference, greedy cover of the x masks by (tile bit set, displacement) passes, staged
chunks within the term and group caps, pieces of oversized groups, the streaming form by classes of high x bits) compiled with g++
alone under ASan + UBSan: tests/cpu/cross_cover_check.cpp replays the plan of every rank the way k_tile_cross / k_tile_cross_real /
k_cross_small / k_cross_small_real index it and compares <phi|H|psi> and H psi with the term-by-term definition to
1e-12 max(1, |c|_1), complex and real flavour."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cross_cover_planner_under_asan_ubsan(tmp_path):
    src = os.path.join(ROOT, "tests", "cpu", "cross_cover_check.cpp")
    exe = str(tmp_path / "cross_cover_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-o", exe, src])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    for seed in ("7", "2025"):
        r = subprocess.run([exe, "40", seed], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "cross cover ok" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
