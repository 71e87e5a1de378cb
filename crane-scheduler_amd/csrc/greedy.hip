// greedy.hip — sequential-greedy batch placement (BASELINE config 5).
//
// One `now` for the batch.  Pods are placed in order; each placement is a new
// Binding{Timestamp: now_unix} on the chosen node, which raises that node's
// window counts (binding.go:85-91: now_unix > now_unix - int64(tr.Seconds())
// iff the window is positive), hence its hot value (node.go:113-121) and
// penalty int(hv*10) (plugins.go:91), before the next pod is scored.  Since
// `now` is fixed, only the chosen node's score changes per step.
//
// G1 greedy_prep: one thread per node — base = int(score/weight) at now
//    (stats.go:114-138, exact int64 path), feasibility (plugins.go:55-66) and
//    the leaf byte = final score | feasible << 7.
// G2 greedy_run: ONE workgroup.  Leaves live in LDS (when they fit beside the
//    levels) or global memory; above them a 64-ary max tree of (max feasible,
//    max any) score pairs in LDS.  Per pod, wave 0 descends the tree with a
//    wave maximum at the root and one ballot per lower level (lowest index wins
//    ties), then updates the chosen node's counts and leaf and re-reduces its
//    ancestors.  Tree, descent and re-reduction are greedy_dev.hpp's, shared
//    with greedy_run_times (why not the commit: see there); this kernel
//    reaches the counts and base[] with plain loads and stores (PlainAccess)
//    and keeps a chunk's 64 results in registers.  The leaves in LDS are not written back: greedy_prep
//    rewrites them before every run.  No atomics, one wave: deterministic.
#include <hip/hip_runtime.h>

#include "dyn_types.hpp"
#include "greedy_dev.hpp"
#include "kernels.hpp"

namespace crane {

template <int PD, int PR>
__global__ __launch_bounds__(256) void greedy_prep(const NodeRec<PD, PR>* __restrict__ rec, int64_t N,
                                                   const uint32_t* __restrict__ cnt, GreedyArgs a,
                                                   int64_t* __restrict__ base_out, uint8_t* __restrict__ leaf) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const NodeRec<PD, PR>& r = rec[n];
    const int64_t base = greedy_base(r, a.now, a);
    const bool feasible = !(a.now < r.e_fail);
    base_out[n] = base;
    leaf[n] = greedy_leaf(base, pen_of(cnt, N, n, a), feasible);
}

template <int NLEV>
__global__ __launch_bounds__(256) void greedy_run(int64_t N, uint8_t* __restrict__ leaf_g, const int64_t* __restrict__ base,
                                                  uint32_t* __restrict__ cnt, GreedyArgs a, int64_t P,
                                                  const uint8_t* __restrict__ flags, int64_t* __restrict__ chosen,
                                                  int32_t leaves_in_lds) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    Tree t;
    tree_layout<NLEV>(t, smem, N, leaves_in_lds);
    uint8_t* leaf = leaves_in_lds ? smem : leaf_g;
    tree_load_build<NLEV, PlainAccess>(t, leaf, leaf_g, N, base, cnt, a.n_win, P, chosen);
    if (wave != 0) return;
    for (int64_t p0 = 0; p0 < P; p0 += 64) {
        const int64_t pl = p0 + lane;
        // DaemonSet pods bypass Filter (plugins.go:41-43): one bit per pod of this chunk
        const uint64_t dsmask = ballot64(pl < P && flags && (flags[pl] & 1u));
        int64_t out = -1;
        const int np = (int)min((int64_t)64, P - p0);
        for (int q = 0; q < np; ++q) {
            const int64_t idx = tree_descend<NLEV>(t, leaf, (dsmask >> q) & 1, lane);
            if (lane == q) out = idx;
            if (idx < 0) continue;
            // ---- commit: Binding{Node: idx, Timestamp: now_unix}
            if (lane == 0) {
                // one round trip: counts and base load together, counts stored back
                uint32_t c[kMaxWin];
#pragma unroll
                for (int w = 0; w < kMaxWin; ++w)
                    if (w < a.n_win) c[w] = cnt[(int64_t)w * N + idx];
                const int64_t b = base[idx];
                int64_t v = 0;
#pragma unroll
                for (int w = 0; w < kMaxWin; ++w) {
                    if (w >= a.n_win) break;
                    c[w] += a.win_inc[w] ? 1u : 0u;
                    cnt[(int64_t)w * N + idx] = c[w];
                    v += win_quot(c[w], a.win_count[w]);
                }
                const uint8_t old = leaf[idx];
                leaf[idx] = (uint8_t)(final_score(b, pen_of_sum(v)) | (old & 0x80));
            }
            // LDS instructions of one wave execute in order, so lane 0's leaf store
            // is seen by the reads below; a global leaf store is waited for.
            if (!leaves_in_lds) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_wave_barrier();
            tree_rereduce<NLEV>(t, leaf, idx, lane);
        }
        if (lane < np) chosen[p0 + lane] = out;
    }
}

template <int PD, int PR>
static hipError_t launch_greedy_t(const void* rec, int64_t N, uint32_t* cnt, const GreedyArgs& a, int64_t* base,
                                  uint8_t* leaf, int64_t P, const uint8_t* flags, int64_t* chosen, hipStream_t st,
                                  int what) {
    if (N > kGreedyMaxNodes) return hipErrorInvalidValue;
    if (N > 0 && (what & kGreedyPrep)) {
        hipError_t e = klaunch("greedy_prep", greedy_prep<PD, PR>, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st,
                               static_cast<const NodeRec<PD, PR>*>(rec), N, cnt, a, base, leaf);
        if (e != hipSuccess) return e;
    }
    if (!(what & kGreedyRun)) return hipSuccess;
    const GreedyTreeShape ts = greedy_tree_shape(N, 0);
    return with_levels(ts.nlev, [&](auto L) {
        return launch_greedy_run<greedy_run<L()>>("greedy_run", ts.lds_bytes, st, N, leaf, base, cnt, a, P, flags,
                                                  chosen, (int32_t)ts.in_lds);
    });
}

hipError_t launch_greedy(int shape, const void* rec, int64_t N, uint32_t* cnt, const GreedyArgs& a, int64_t* base,
                         uint8_t* leaf, int64_t P, const uint8_t* flags, int64_t* chosen, hipStream_t st, int what) {
    return with_shape(shape, [&](auto pd, auto pr) {
        return launch_greedy_t<pd(), pr()>(rec, N, cnt, a, base, leaf, P, flags, chosen, st, what);
    });
}

}  // namespace crane
