"""CPU test of the wave-sum networks of the batched sparse kernels (openvqe_amd/csrc/sv_wave_reduce.hpp): the host instantiation
over arrays of 64 lanes, tests/cpu/wave_reduce_check.cpp, under ASan + UBSan with g++ alone — lane 8 q of the transposed
eight-state network and lane 0 of the single-value form against the __shfl_down tree of wave_sum, bit for bit."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wave_sum_networks_keep_the_bits_of_the_shfl_down_tree(tmp_path):
    src = os.path.join(ROOT, "tests", "cpu", "wave_reduce_check.cpp")
    exe = str(tmp_path / "wave_reduce_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-o", exe, src])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    for seed in ("7", "2025"):
        r = subprocess.run([exe, seed], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "wave reduce ok" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
