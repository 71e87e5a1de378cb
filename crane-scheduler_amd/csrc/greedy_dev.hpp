// greedy_dev.hpp — device functions the sequential-greedy kernels share: greedy_prep and
// greedy_run (greedy.hip) and greedy_run_times (greedy_times.hip).  A node's base score, its
// penalty from the window counts and its leaf byte are stated here once, so the kernel that
// recomputes a node between two pods uses the instructions the preparation used.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dyn_types.hpp"
#include "kernels.hpp"

namespace crane {

__device__ __forceinline__ int64_t go_int_g(double x) {
    if (!(x >= -9223372036854775808.0 && x < 9223372036854775808.0)) return INT64_MIN;
    return (int64_t)x;
}

__device__ __forceinline__ int32_t final_score(int64_t base, int64_t pen) {
    const int64_t f = (int64_t)((uint64_t)base - (uint64_t)pen);  // Go int64 wraps
    return (int32_t)(f < 0 ? 0 : (f > 100 ? 100 : f));
}

// one window's term of the hot value: Go int division truncates toward zero; 32-bit unsigned
// division when it is the same thing
__device__ __forceinline__ int64_t win_quot(uint32_t c, int64_t k) {
    return (k > 0 && k <= 0xFFFFFFFFll) ? (int64_t)(c / (uint32_t)k) : (int64_t)c / k;
}

// the penalty int(hv * 10) of the summed terms (node.go:117, plugins.go:91)
__device__ __forceinline__ int64_t pen_of_sum(int64_t v) {
    if (v < 0) return 0;  // a negative annotation is rejected (stats.go:71-73) -> hot value 0
    return go_int_g((double)v * 10.0);
}

// hot value of a node from its per-window counts (node.go:113-121)
__device__ __forceinline__ int64_t pen_of(const uint32_t* cnt, int64_t N, int64_t n, const GreedyArgs& a) {
    int64_t v = 0;
    for (int w = 0; w < a.n_win; ++w) v += win_quot(cnt[(int64_t)w * N + n], a.win_count[w]);
    return pen_of_sum(v);
}

// base = int(score / weight) of a node at `now` (stats.go:114-138): the priorities' terms whose
// metric is fresh, summed in policy order in fp64, then one division
template <int PD, int PR>
__device__ __forceinline__ int64_t greedy_base(const NodeRec<PD, PR>& r, int64_t now, const GreedyArgs& a) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < PR; ++k)
        if (now < r.e_prio[k]) s += r.t[k];
    return a.noprio ? 0 : go_int_g(s / a.wsum);
}

__device__ __forceinline__ uint8_t greedy_leaf(int64_t base, int64_t pen, bool feasible) {
    return (uint8_t)(final_score(base, pen) | (feasible ? 0x80 : 0));
}

// ---- wave helpers (64 lanes)
__device__ __forceinline__ uint64_t ballot64(bool p) { return __ballot(p); }

// max over lanes of v in [0, 127] and the lowest lane holding it; v < 0 lanes never win
__device__ __forceinline__ int wave_argmax7(int v, int* lane_out) {
    uint64_t cand = ballot64(v >= 0);
    if (!cand) {
        *lane_out = -1;
        return -1;
    }
    int m = 0;
#pragma unroll
    for (int b = 6; b >= 0; --b) {
        const uint64_t with = cand & ballot64((v >> b) & 1);
        if (with) {
            cand = with;
            m |= 1 << b;
        }
    }
    *lane_out = __builtin_ctzll(cand);
    return m;
}

// wave max via DPP: row_shr 1,2,4,8 then row_bcast15/31 (GFX9 family) -> lane 63.
// Out-of-range source lanes return `old` = v itself, the identity of max.
__device__ __forceinline__ int wave_max_dpp(int v) {
    v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x111, 0xF, 0xF, false));  // row_shr:1
    v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x112, 0xF, 0xF, false));  // row_shr:2
    v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x114, 0xF, 0xF, false));  // row_shr:4
    v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x118, 0xF, 0xF, false));  // row_shr:8
    v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x142, 0xA, 0xF, false));  // row_bcast:15
    v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x143, 0xC, 0xF, false));  // row_bcast:31
    return __builtin_amdgcn_readlane(v, 63);
}

constexpr int kGreedyLevels = 4;  // 64^4 = 16.7M nodes

struct Tree {
    int nlev;                     // internal levels above the leaves (>= 1)
    int64_t size[kGreedyLevels + 1];  // entries per level, level 0 = leaves
    uint16_t* lvl[kGreedyLevels + 1]; // LDS arrays for levels >= 1: lo byte max-any, hi byte max-feasible+1
};

__device__ __forceinline__ int leaf_val(uint8_t b, bool any) {
    const int sc = b & 0x7F;
    return any ? sc : ((b & 0x80) ? sc : -1);
}
__device__ __forceinline__ int ent_val(uint16_t e, bool any) { return any ? (int)(e & 0xFF) : (int)(e >> 8) - 1; }

}  // namespace crane
