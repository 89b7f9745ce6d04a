// sv_wave_reduce.hpp — wave sums of the batched sparse kernels on the VALU lane exchanges of gfx950, with the association of
// wave_sum (sv_kernels.hpp).
//
// wave_sum is six __shfl_down steps, v += v[lane + off] for off = 32, 16, 8, 4, 2, 1; its total is read in lane 0.  On a double
// every step is two ds_bpermute_b32 and a wait for them: six dependent LDS round trips per sum.  Lane 0's total is a fixed tree,
//   a_l = v_l + v_{l+32} (l < 32),  b_l = a_l + a_{l+16} (l < 16),  c_l = b_l + b_{l+8},  d_l = c_l + c_{l+4},  e_l = d_l + d_{l+2},
//   f_0 = e_0 + e_1,
// and the networks below compute the SAME tree — every addition has the same two operands, so every total keeps its bits — with
// v_permlane32_swap / v_permlane16_swap and DPP row operations: the values never leave the VGPRs.
//
//   wave_sums8       eight sums at once, TRANSPOSED: at each of the first three levels half of the lanes take over half of the
//                    states, so that a level costs half the additions of the one before instead of eight every time.  The total
//                    of state q comes out in lane 8 q (no other lane holds anything meaningful).
//   wave_sum_lane0   one sum, same tree; the total comes out in lane 0.
//
// Both are written ONCE over an exchange policy X — X::V is "one register of all lanes" — so that the same source runs on the
// device (WaveLanes: V = double, the builtins) and on the host over arrays of 64 lanes (tests/cpu/wave_reduce_check.cpp), where
// it is compared bit for bit with the __shfl_down tree written out.  A policy provides, with rows of 16 lanes:
//   swap32(a, b)    lanes 32-63 of a <-> lanes 0-31 of b                      (v_permlane32_swap a, b)
//   swap16(a, b)    rows 1, 3 of a <-> rows 0, 2 of b                        (v_permlane16_swap a, b)
//   ror8(v)         lane i <- lane i ^ 8                                     (DPP row_ror:8)
//   shl<N>(v)       lane i <- lane i + N of the same row, 0 past its end     (DPP row_shl:N)
//   pick8(a, b)     lane & 8 ? a : b
//   add(a, b)       a + b in every lane
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define OVQE_WR_HD __host__ __device__ __forceinline__
#else
#define OVQE_WR_HD inline
#endif

namespace ovqe {

// acc[q]: the addends of state q, one per lane.  -> z: lane 8 q holds the total of state q.  acc is consumed.
template <class X>
OVQE_WR_HD typename X::V wave_sums8(const X &x, typename X::V (&acc)[8]) {
    using V = typename X::V;
    // level 32: lanes 0-31 keep states 0..3, lanes 32-63 states 4..7; every lane holds v_l + v_{l+32} of its four
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        x.swap32(acc[j], acc[4 + j]);
        acc[j] = x.add(acc[j], acc[4 + j]);
    }
    // level 16: row 0 keeps states 0, 1, row 1 states 2, 3, row 2 states 4, 5, row 3 states 6, 7
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        x.swap16(acc[j], acc[2 + j]);
        acc[j] = x.add(acc[j], acc[2 + j]);
    }
    // level 8: the lower octet of a row keeps the row's first state, the upper octet its second
    const V p = x.pick8(acc[1], acc[0]), s = x.pick8(acc[0], acc[1]);
    V z = x.add(p, x.ror8(s));
    // levels 4, 2, 1 inside the octet
    z = x.add(z, x.template shl<4>(z));
    z = x.add(z, x.template shl<2>(z));
    z = x.add(z, x.template shl<1>(z));
    return z;
}

// -> lane 0 holds the total of v over the wave
template <class X>
OVQE_WR_HD typename X::V wave_sum_lane0(const X &x, typename X::V v) {
    using V = typename X::V;
    V t = v;
    x.swap32(v, t);   // v: [v_lo | v_lo], t: [v_hi | v_hi]
    v = x.add(v, t);
    t = v;
    x.swap16(v, t);   // row 0 of v: its own, row 0 of t: row 1
    v = x.add(v, t);
    v = x.add(v, x.template shl<8>(v));
    v = x.add(v, x.template shl<4>(v));
    v = x.add(v, x.template shl<2>(v));
    v = x.add(v, x.template shl<1>(v));
    return v;
}

#if defined(__HIPCC__)
// the device policy: one double per lane.  Every lane of the wave must be active.  (The compiler inserts the wait states between
// a VALU write and a permlane swap or DPP read of the same register itself.)
struct WaveLanes {
    using V = double;
    int lane;
    template <int CTRL>
    __device__ __forceinline__ static double dpp(double v) {
        const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, false);
        const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, false);
        return __hiloint2double(hi, lo);
    }
    __device__ __forceinline__ void swap32(double &a, double &b) const {
        const auto lo = __builtin_amdgcn_permlane32_swap((unsigned)__double2loint(a), (unsigned)__double2loint(b), false, false);
        const auto hi = __builtin_amdgcn_permlane32_swap((unsigned)__double2hiint(a), (unsigned)__double2hiint(b), false, false);
        a = __hiloint2double((int)hi[0], (int)lo[0]);
        b = __hiloint2double((int)hi[1], (int)lo[1]);
    }
    __device__ __forceinline__ void swap16(double &a, double &b) const {
        const auto lo = __builtin_amdgcn_permlane16_swap((unsigned)__double2loint(a), (unsigned)__double2loint(b), false, false);
        const auto hi = __builtin_amdgcn_permlane16_swap((unsigned)__double2hiint(a), (unsigned)__double2hiint(b), false, false);
        a = __hiloint2double((int)hi[0], (int)lo[0]);
        b = __hiloint2double((int)hi[1], (int)lo[1]);
    }
    __device__ __forceinline__ double ror8(double v) const { return dpp<0x128>(v); }
    template <int N>
    __device__ __forceinline__ double shl(double v) const {
        static_assert(N >= 1 && N <= 15, "row_shl:N");
        return dpp<0x100 + N>(v);
    }
    __device__ __forceinline__ double pick8(double a, double b) const { return (lane & 8) ? a : b; }
    __device__ __forceinline__ double add(double a, double b) const { return a + b; }
};
#endif

}  // namespace ovqe
