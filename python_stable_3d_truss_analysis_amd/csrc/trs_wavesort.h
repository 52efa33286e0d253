// Ascending sort of 64 R unsigned 32-bit keys by ONE wave, the keys in registers: a bitonic network.
//
// Layout: key i of the 64 R sits in register i / 64 of lane i % 64 - before the sort (the caller fills v[r] of lane l
// with key 64 r + l, padding with 0xffffffff) and after it (v[r] of lane l is the key of rank 64 r + l, so a store of
// register r is one contiguous run of 64 elements).  A compare-exchange at distance j < 64 takes the partner's key
// with a lane exchange (lane ^ j: DPP inside a quad, ds_swizzle up to 16, a shuffle for 32) and keeps the minimum or
// the maximum by the lane's side; at distance j >= 64 the partner is register r ^ (j / 64) of the same lane - a min /
// max pair, no exchange.  The direction of a merge of length K is ascending where bit K of i is clear: a lane bit for
// K < 64, a register bit known at compile time from K = 64 on.
//
// log2(64 R) (log2(64 R) + 1) / 2 steps: 21, 28, 36, 45 for R = 1, 2, 4, 8, of which 21 + 6 log2(R) cross lanes.  No
// LDS, no barrier; every lane of the wave must be active.  Any ascending sort of DISTINCT keys gives the same array,
// which is what the callers rely on (csrc/order.hip: the position in the id list sits in a key's low bits).
#pragma once
#include <hip/hip_runtime.h>

namespace trs_wavesort {

template <int J>
__device__ __forceinline__ unsigned lane_xor(unsigned v) {   // the value of lane (lane ^ J)
    static_assert(J == 1 || J == 2 || J == 4 || J == 8 || J == 16 || J == 32, "a single lane bit");
    if constexpr (J == 1)
        return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, false);   // quad_perm [1, 0, 3, 2]
    else if constexpr (J == 2)
        return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, false);   // quad_perm [2, 3, 0, 1]
    else if constexpr (J <= 16)
        return (unsigned)__builtin_amdgcn_ds_swizzle((int)v, (J << 10) | 0x1f);           // bit mode: and 0x1f, or 0, xor J
    else
        return (unsigned)__shfl_xor((int)v, 32);
}

// one compare-exchange step of the merge of length K at distance J
template <int R, int K, int J>
__device__ __forceinline__ void step(unsigned (&v)[R], const int lane) {
    if constexpr (J >= 64) {
        constexpr int D = J / 64;
#pragma unroll
        for (int r = 0; r < R; ++r)
            if ((r & D) == 0) {
                const unsigned lo = min(v[r], v[r + D]), hi = max(v[r], v[r + D]);
                const bool asc = ((64 * r) & K) == 0;
                v[r] = asc ? lo : hi;
                v[r + D] = asc ? hi : lo;
            }
    } else {
        const bool lower = (lane & J) == 0;                                   // this lane holds the smaller index of the pair
        const bool keep_min = K < 64 ? lower == ((lane & K) == 0) : lower;    // ... in an ascending merge
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const unsigned other = lane_xor<J>(v[r]);
            const unsigned lo = min(v[r], other), hi = max(v[r], other);
            const bool asc = K < 64 || ((64 * r) & K) == 0;
            // (one compare, the agreement with keep_min on the scalar unit and one select - two vector instructions
            // instead of three - measured 3 % SLOWER on the whole kernel: EXPERIMENTS R25)
            v[r] = (asc ? keep_min : !keep_min) ? lo : hi;
        }
    }
}

template <int R, int K, int J>
__device__ __forceinline__ void merge(unsigned (&v)[R], const int lane) {
    step<R, K, J>(v, lane);
    if constexpr (J > 1) merge<R, K, J / 2>(v, lane);
}

template <int R, int K = 2>
__device__ __forceinline__ void sort(unsigned (&v)[R], const int lane) {
    static_assert(R == 1 || R == 2 || R == 4 || R == 8, "64, 128, 256 or 512 keys");
    merge<R, K, K / 2>(v, lane);
    if constexpr (K < 64 * R) sort<R, 2 * K>(v, lane);
}

}  // namespace trs_wavesort
