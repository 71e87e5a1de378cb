// wave.hpp — the wave primitives and the packed keys every kernel shares.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace crane {

// A list key (score << 24 | 0xFFFFFF - node index within the producer's range, -1 = the pod may not
// go there) and the key a pod's result carries: (score << 32) | (0xFFFFFFFF - global node), the
// inverse of crane_dyn_key_node.  Larger = better; the lowest index wins ties.
__host__ __device__ __forceinline__ int32_t pack_key(int32_t f, int64_t n) { return (f << 24) | (int32_t)(0xFFFFFF - n); }
__host__ __device__ __forceinline__ long long wide_key(int64_t score, int64_t global_node) {
    return (long long)((score << 32) | (int64_t)(0xFFFFFFFFull - (uint64_t)global_node));
}
// a list key >= 0 of a range that starts at global node g0
__host__ __device__ __forceinline__ long long wide_key_of(int32_t k, int64_t g0) {
    return wide_key(k >> 24, g0 + (0xFFFFFF - (k & 0xFFFFFF)));
}

// one bit per lane of the 64-lane wave
__device__ __forceinline__ uint64_t ballot64(bool p) { return __ballot(p); }

// ---- on DPP (VALU lane moves, no LDS round trip like ds_bpermute's __shfl*).  Every lane of the
// 64-lane wave must be active (uniform control flow).
// dpp_ctrl: quad_perm 0x00-0xFF, row_shr:k 0x110 + k, row_ror:k 0x120 + k, row_bcast:15 0x142,
// row_bcast:31 0x143; lanes whose source is outside the row keep `id` (bound_ctrl off).
template <int CTRL, int ROWS = 0xF>
__device__ __forceinline__ int32_t dpp_or(int32_t id, int32_t v) {
    return __builtin_amdgcn_update_dpp(id, v, CTRL, ROWS, 0xF, false);
}
// maximum over the wave, uniform
__device__ __forceinline__ int32_t wave_max(int32_t v) {
    v = max(v, dpp_or<0xB1>(v, v));   // quad_perm [1,0,3,2]
    v = max(v, dpp_or<0x4E>(v, v));   // quad_perm [2,3,0,1]
    v = max(v, dpp_or<0x124>(v, v));  // row_ror:4
    v = max(v, dpp_or<0x128>(v, v));  // row_ror:8: every lane holds its row's maximum
    return max(max(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
               max(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}
// the same as a shift-and-broadcast chain ending in one readlane: row_shr 1, 2, 4, 8, then
// row_bcast:15 / :31 carry the rows' maxima up to lane 63 (lanes without a source keep v, the
// identity of max).  The sequential greedy kernels' form (greedy_dev.hpp): their registers and
// their time per pod were measured with it.
__device__ __forceinline__ int32_t wave_max_shr(int32_t v) {
    v = max(v, dpp_or<0x111>(v, v));
    v = max(v, dpp_or<0x112>(v, v));
    v = max(v, dpp_or<0x114>(v, v));
    v = max(v, dpp_or<0x118>(v, v));
    v = max(v, dpp_or<0x142, 0xA>(v, v));
    v = max(v, dpp_or<0x143, 0xC>(v, v));
    return __builtin_amdgcn_readlane(v, 63);
}
// the same through ds_bpermute shuffles, for K3m (matrix.hip): the DPP form costs its one-node
// instances 2 to 4 VGPRs, and the 8 x 8 ones an occupancy step
__device__ __forceinline__ int32_t wave_max_shfl(int32_t v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}
// inclusive prefix (lane order) under an associative op with identity id: Hillis-Steele
// within each row of 16, then rows 1 / 3 take row 0 / 2's total, rows 2-3 rows 0-1's
template <class Op>
__device__ __forceinline__ int32_t wave_scan(int32_t v, int32_t id, Op op) {
    v = op(v, dpp_or<0x111>(id, v));
    v = op(v, dpp_or<0x112>(id, v));
    v = op(v, dpp_or<0x114>(id, v));
    v = op(v, dpp_or<0x118>(id, v));
    v = op(v, dpp_or<0x142, 0xA>(id, v));
    v = op(v, dpp_or<0x143, 0xC>(id, v));
    return v;
}
__device__ __forceinline__ uint32_t wave_scan_add(uint32_t v) {
    return (uint32_t)wave_scan((int32_t)v, 0, [](int32_t a, int32_t b) { return (int32_t)((uint32_t)a + (uint32_t)b); });
}
__device__ __forceinline__ int32_t wave_scan_max(int32_t v) {
    return wave_scan(v, INT32_MIN, [](int32_t a, int32_t b) { return max(a, b); });
}
// lane i takes lane (i ^ 1)'s value / lane i + 2's within its quad (lanes 0, 1 of a quad)
__device__ __forceinline__ int32_t quad_xor1(int32_t v) { return dpp_or<0xB1>(v, v); }
__device__ __forceinline__ int32_t quad_down2(int32_t v) { return dpp_or<0xEE>(v, v); }

// ---- 64-bit values (butterflies through __shfl_xor): every lane gets the wave's result
__device__ __forceinline__ long long wave_max64(long long v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = max(v, (long long)__shfl_xor(v, o));
    return v;
}
// mn, mx: the wave's minimum of mn and maximum of mx
__device__ __forceinline__ void wave_minmax64(int64_t& mn, int64_t& mx) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        mn = min(mn, (int64_t)__shfl_xor((long long)mn, o));
        mx = max(mx, (int64_t)__shfl_xor((long long)mx, o));
    }
}
// a 64-bit value of lane j / of the first active lane, uniform
__device__ __forceinline__ int64_t readlane64(int64_t v, int j) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, j);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), j);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ int64_t readfirstlane64(int64_t v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

}  // namespace crane
