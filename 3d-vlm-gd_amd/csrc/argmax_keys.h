// Packed (score, index) argmax keys shared by the evaluation kernels (match.hip, track.hip).
// The unsigned maximum of orderable(score) << 32 | ~index is the larger score, and of equal scores the smaller index
// (torch.argmax's first occurrence) — a max, so the result does not depend on the order in which tiles, waves or atomics
// combine.
#pragma once
#include "gd_common.h"

__device__ __forceinline__ unsigned gd_ord(float v) {
    const unsigned u = gd_f2u(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float gd_unord(unsigned o) {
    return __builtin_bit_cast(float, (o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}
__device__ __forceinline__ unsigned long long gd_key(float v, int idx) {
    return ((unsigned long long)gd_ord(v) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)idx);
}
// the index a key was made with
__device__ __forceinline__ int gd_key_index(unsigned long long k) { return (int)(0xFFFFFFFFu - (unsigned)(k & 0xFFFFFFFFull)); }
__device__ __forceinline__ unsigned long long umax64(unsigned long long a, unsigned long long b) { return a > b ? a : b; }
template <int CTRL> __device__ __forceinline__ unsigned long long dpp_u64(unsigned long long v) {
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)v, CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(v >> 32), CTRL, 0xF, 0xF, false);
    return ((unsigned long long)(unsigned)hi << 32) | (unsigned long long)(unsigned)lo;
}
// max over each row of 16 lanes (DPP: quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror), result in every lane of the row
__device__ __forceinline__ unsigned long long row16_max_u64(unsigned long long v) {
    v = umax64(v, dpp_u64<0xB1>(v));
    v = umax64(v, dpp_u64<0x4E>(v));
    v = umax64(v, dpp_u64<0x141>(v));
    v = umax64(v, dpp_u64<0x140>(v));
    return v;
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = umax64(v, __shfl_xor(v, o, 64));
    return v;
}
