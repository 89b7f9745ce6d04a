// wave_reduce_check.cpp — the wave-sum networks of openvqe_amd/csrc/sv_wave_reduce.hpp instantiated on the HOST over arrays of 64
// lanes, compiled alone with g++ (ASan + UBSan in tests/test_wave_reduce.py).  The exchange policy below states the lane semantics
// of v_permlane32_swap, v_permlane16_swap and the DPP row operations as the kernels assume them (rows of 16 lanes); the networks
// are the same source the kernels run.  Random doubles of both signs and mixed magnitudes (so that the order of the additions
// shows in the last bits): for each of the 8 states the value in lane 8 q of wave_sums8, and lane 0 of wave_sum_lane0, must equal
// BIT FOR BIT lane 0 of the six __shfl_down steps of wave_sum (sv_kernels.hpp) written out.  No other lane is read.
// What this cannot check is that the hardware exchanges lanes as the policy says: tests/test_gpu_sparse_reduce.py does, against
// the __shfl_down kernels on the device.
//   usage: wave_reduce_check [seed]
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <utility>

#include "../../openvqe_amd/csrc/sv_wave_reduce.hpp"

using namespace ovqe;

struct Lanes {
    double v[64];
};

struct HostLanes {
    using V = Lanes;
    void swap32(Lanes &a, Lanes &b) const {
        for (int l = 0; l < 32; ++l) std::swap(a.v[32 + l], b.v[l]);
    }
    void swap16(Lanes &a, Lanes &b) const {   // odd rows of the first operand <-> even rows of the second
        for (int row = 0; row < 4; row += 2)
            for (int l = 0; l < 16; ++l) std::swap(a.v[16 * (row + 1) + l], b.v[16 * row + l]);
    }
    Lanes ror8(const Lanes &s) const {
        Lanes r;
        for (int l = 0; l < 64; ++l) r.v[l] = s.v[(l & ~15) | ((l + 8) & 15)];
        return r;
    }
    template <int N>
    Lanes shl(const Lanes &s) const {
        Lanes r;
        for (int l = 0; l < 64; ++l) r.v[l] = (l & 15) + N < 16 ? s.v[l + N] : 0.0;   // (no source lane: the old value, 0)
        return r;
    }
    Lanes pick8(const Lanes &a, const Lanes &b) const {
        Lanes r;
        for (int l = 0; l < 64; ++l) r.v[l] = (l & 8) ? a.v[l] : b.v[l];
        return r;
    }
    Lanes add(const Lanes &a, const Lanes &b) const {
        Lanes r;
        for (int l = 0; l < 64; ++l) r.v[l] = a.v[l] + b.v[l];
        return r;
    }
};

// wave_sum: v += __shfl_down(v, off, 64) — a lane whose source is past the wave reads its own value
static double shfl_down_tree(const Lanes &in) {
    Lanes v = in;
    for (int off = 32; off > 0; off >>= 1) {
        Lanes n;
        for (int l = 0; l < 64; ++l) n.v[l] = v.v[l] + (l + off < 64 ? v.v[l + off] : v.v[l]);
        v = n;
    }
    return v.v[0];
}

static uint64_t bits(double x) {
    uint64_t u;
    std::memcpy(&u, &x, sizeof u);
    return u;
}

int main(int argc, char **argv) {
    const unsigned seed = argc > 1 ? (unsigned)std::strtoul(argv[1], nullptr, 10) : 1u;
    std::mt19937_64 rng(seed);
    std::uniform_real_distribution<double> mant(-1.0, 1.0);
    std::uniform_int_distribution<int> expo(-40, 12), kind(0, 9);
    int fails = 0, rounded = 0;
    const int trials = 2000;
    for (int t = 0; t < trials; ++t) {
        // trial kinds: mixed magnitudes (most), equal magnitudes, a few exact zeros, one dominant lane
        const int k = kind(rng);
        Lanes acc[8];
        double want[8];
        for (int q = 0; q < 8; ++q) {
            for (int l = 0; l < 64; ++l) {
                double x = std::ldexp(mant(rng), k == 0 ? 0 : expo(rng));
                if (k == 1 && (rng() & 3) == 0) x = 0.0;
                acc[q].v[l] = x;
            }
            if (k == 2) acc[q].v[rng() & 63] = std::ldexp(mant(rng), 30);
            want[q] = shfl_down_tree(acc[q]);
            // (the order matters for these inputs: the plain left-to-right sum differs in most trials)
            double plain = 0.0;
            for (int l = 0; l < 64; ++l) plain += acc[q].v[l];
            rounded += bits(plain) != bits(want[q]);
        }
        const HostLanes x;
        for (int q = 0; q < 8; ++q) {
            const Lanes one = wave_sum_lane0(x, acc[q]);
            if (bits(one.v[0]) != bits(want[q])) {
                std::printf("FAIL trial %d state %d: wave_sum_lane0 %a, __shfl_down tree %a\n", t, q, one.v[0], want[q]);
                if (++fails > 20) return 1;
            }
        }
        const Lanes z = wave_sums8(x, acc);
        for (int q = 0; q < 8; ++q) {
            if (bits(z.v[8 * q]) != bits(want[q])) {
                std::printf("FAIL trial %d state %d: wave_sums8 lane %d %a, __shfl_down tree %a\n", t, q, 8 * q, z.v[8 * q], want[q]);
                if (++fails > 20) return 1;
            }
        }
    }
    if (rounded < trials) {   // of 8 * trials sums
        std::printf("FAIL: the inputs do not tell one order of additions from another (%d of %d sums)\n", rounded, 8 * trials);
        return 1;
    }
    if (fails) return 1;
    std::printf("wave reduce ok: %d trials of 8 sums, seed %u; %d sums differ from the left-to-right sum\n", trials, seed, rounded);
    return 0;
}
