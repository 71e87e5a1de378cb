// greedy_dev.hpp — what the sequential-greedy kernels share: greedy_prep and greedy_run
// (greedy.hip) and greedy_run_times (greedy_times.hip).
//  * A node's base score, its penalty from the window counts and its leaf byte, stated once, so
//    the kernel that recomputes a node between two pods uses the instructions the preparation used.
//  * The one-workgroup core of the two run kernels: the 64-ary max tree over the leaf bytes (layout,
//    load and build), the per-pod descent and the re-reduction of the chosen leaf's ancestors.
//    The kernels keep their per-pod loops; how they reach the counts and base[] is an access
//    policy (PlainAccess, WgAccess).
//  * NOT the commit's loads and stores, which stay written out in each kernel over win_quot and
//    pen_of_sum.  As a function taking the GreedyArgs, the compiler (ROCm 7.2) moves every loaded
//    count to a scalar register as it arrives: one memory round trip per window where the
//    kernels have one in all, measured at +17 to +21 % per pod in greedy_run and +4 to +6 % in
//    greedy_run_times (profiles/ab/greedy_core_refactor.txt).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dyn_types.hpp"
#include "kernels.hpp"
#include "node_rec.hpp"
#include "wave.hpp"

namespace crane {

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
    return go_int((double)v * 10.0);
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
    return a.noprio ? 0 : go_int(s / a.wsum);
}

__device__ __forceinline__ uint8_t greedy_leaf(int64_t base, int64_t pen, bool feasible) {
    return (uint8_t)(final_score(base, pen) | (feasible ? 0x80 : 0));
}

// ---- how a run kernel reaches the counts and base[].  greedy_run: plain loads and stores.
// greedy_run_times also decrements the counts with atomics, so its other accesses to them (and to
// the base[] entries it rewrites) are relaxed workgroup-scope atomic accesses: the kernel is one
// workgroup, and the loads still hit L1 as plain loads do.
struct PlainAccess {
    template <class T>
    static __device__ __forceinline__ T ld(const T* p) { return *p; }
};
struct WgAccess {
    template <class T>
    static __device__ __forceinline__ T ld(const T* p) {
        return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    template <class T>
    static __device__ __forceinline__ void st(T* p, T v) {
        __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
};

// ---- the 64-ary max tree.  Level 0 is the leaf bytes (score | feasible << 7; in LDS when they
// fit, else in global memory), level l >= 1 an LDS array of one entry per 64 children.
constexpr int kGreedyLevels = 4;  // the most levels >= 1 (with_levels); kGreedyMaxNodes = 64^4 needs 3

struct Tree {
    int64_t size[kGreedyLevels + 1];   // entries per level
    uint16_t* lvl[kGreedyLevels + 1];  // levels >= 1: lo byte max-any, hi byte max-feasible + 1
};

__device__ __forceinline__ int leaf_val(uint8_t b, bool any) {
    const int sc = b & 0x7F;
    return any ? sc : ((b & 0x80) ? sc : -1);
}
__device__ __forceinline__ int ent_val(uint16_t e, bool any) { return any ? (int)(e & 0xFF) : (int)(e >> 8) - 1; }

// entry c of level l: the maximum below it for a DaemonSet pod (any) or for the others, -1 = none
__device__ __forceinline__ int child_val(const Tree& t, const uint8_t* leaf, int l, int64_t c, bool any) {
    return l == 0 ? leaf_val(leaf[c], any) : ent_val(t.lvl[l][c], any);
}
// a level entry of the two maxima over its children (-1 = none); the lo byte never goes below 0
__device__ __forceinline__ uint16_t tree_entry(int ma, int mf) { return (uint16_t)(max(ma, 0) | ((mf + 1) << 8)); }

// Layout in dynamic LDS: [leaves (if in LDS)] [level 1] [level 2] ...; returns the byte offset
// behind the last level.  Every index into t.size / t.lvl is a compile-time constant in the
// functions below (their level loops are fully unrolled), so the metadata stays in registers.
template <int NLEV>
__device__ __forceinline__ int64_t tree_layout(Tree& t, unsigned char* smem, int64_t N, int32_t leaves_in_lds) {
    int64_t off = leaves_in_lds ? (N + 15) / 16 * 16 : 0, sz = N;
    t.size[0] = N;
#pragma unroll
    for (int l = 1; l <= NLEV; ++l) {
        sz = (sz + 63) / 64;
        t.size[l] = sz;
        t.lvl[l] = reinterpret_cast<uint16_t*>(smem + off);
        off += (sz * 2 + 15) / 16 * 16;
    }
    return off;
}

// Whole workgroup: the leaves into LDS (leaf != leaf_g), the L2 warm-up, the levels bottom-up.
// P and chosen only serve the warm-up's keep-alive store.
template <int NLEV, class Access>
__device__ __forceinline__ void tree_load_build(const Tree& t, uint8_t* leaf, const uint8_t* leaf_g, int64_t N,
                                                const int64_t* base, const uint32_t* cnt, int n_win, int64_t P,
                                                int64_t* chosen) {
    if (leaf != leaf_g)
        for (int64_t i = threadIdx.x; i < N; i += blockDim.x) leaf[i] = leaf_g[i];
    // Warm this XCD's L2 with the per-node state the commits touch (base, counts):
    // most placements hit a node for the first time, which would otherwise be an
    // HBM-latency miss on the serial path.  The xor keeps the loads live.
    {
        uint64_t x = 0;
        for (int64_t i = threadIdx.x; i < N; i += blockDim.x) {
            x ^= (uint64_t)Access::ld(&base[i]);
            for (int w = 0; w < n_win; ++w) x ^= Access::ld(&cnt[(int64_t)w * N + i]);
        }
        if (x == 0x9E3779B97F4A7C15ull && P < 0) chosen[0] = (int64_t)x;  // never true: keeps the loads
    }
    __syncthreads();
    // level 1 from the leaves, then each level from the one below
#pragma unroll
    for (int l = 1; l <= NLEV; ++l) {
        for (int64_t e = threadIdx.x; e < t.size[l]; e += blockDim.x) {
            int ma = 0, mf = -1;
            for (int j = 0; j < 64; ++j) {
                const int64_t c = e * 64 + j;
                if (c >= t.size[l - 1]) break;
                ma = max(ma, child_val(t, leaf, l - 1, c, true));
                mf = max(mf, child_val(t, leaf, l - 1, c, false));
            }
            t.lvl[l][e] = tree_entry(ma, mf);
        }
        __syncthreads();
    }
}

// One wave, all 64 lanes: the best node for a pod (any: a DaemonSet pod, which bypasses Filter),
// lowest index on ties, or -1.  The root level (<= 64 entries), then one ballot per level.
template <int NLEV>
__device__ __forceinline__ int64_t tree_descend(const Tree& t, const uint8_t* leaf, bool any, int lane) {
    const int v = lane < t.size[NLEV] ? ent_val(t.lvl[NLEV][lane], any) : -1;
    const int M = wave_max_shr(v);
    if (M < 0) return -1;
    int64_t idx = __builtin_ctzll(ballot64(v == M));
#pragma unroll
    for (int l = NLEV - 1; l >= 0; --l) {
        const int64_t c = idx * 64 + lane;
        const int w = c < t.size[l] ? child_val(t, leaf, l, c, any) : -1;
        idx = idx * 64 + __builtin_ctzll(ballot64(w == M));
    }
    return idx;
}

// One wave, all 64 lanes: re-reduce the ancestors of leaf idx; stop once an entry is unchanged.
// The leaf's store must be visible to the wave: LDS instructions of one wave execute in order, a
// global leaf store is waited for by the caller.
template <int NLEV>
__device__ __forceinline__ void tree_rereduce(const Tree& t, const uint8_t* leaf, int64_t idx, int lane) {
    int64_t child = idx;
#pragma unroll
    for (int l = 1; l <= NLEV; ++l) {
        const int64_t e = child / 64, c = e * 64 + lane;
        int va = -1, vf = -1;
        if (c < t.size[l - 1]) {
            va = child_val(t, leaf, l - 1, c, true);
            vf = child_val(t, leaf, l - 1, c, false);
        }
        const uint16_t ne = tree_entry(wave_max_shr(va), wave_max_shr(vf));
        const uint16_t oe = t.lvl[l][e];
        if (ne == oe) break;
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) t.lvl[l][e] = ne;
        __builtin_amdgcn_wave_barrier();
        child = e;
    }
}

}  // namespace crane
