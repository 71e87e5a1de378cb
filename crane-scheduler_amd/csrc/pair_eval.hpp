// pair_eval.hpp — the lane cache of the kernels that evaluate (pod, node) pairs from the node
// records: K3m (matrix.hip), the top-k candidates (topk.hip) and the selection's pair kernel
// (select.hip).
//
// For a node, Filter and Score depend on the pod only through `now < expiry` comparisons
// (stats.go:42-48), so whatever a kernel derives from them — its value V — is constant on
// [lo, hi), the interval between the node's consecutive expiries around the evaluation time
// (bracket, step_node.hpp).  A lane evaluates its node at the minimum time cmin of a 64-pod
// sub-chunk whose times are [cmin, cmax] and keeps the value with the interval; a later sub-chunk
// that lies inside the interval reuses it (two 64-bit compares).  A node with one expiry inside
// (cmin, cmax] also holds its value from that expiry bp on (per pod: compare + select); one with
// several is `multi`: its record is read again and evaluated at the pod's own time.
//
// The value and its evaluation are the kernel's: eval(t, record) -> V, calling score_at or key_of.
// No score or Filter arithmetic is restated here.  PairCache serves the kernels whose lanes own one
// node (top-k: the node's two keys; selection: Filter pass and score).  K3m keeps the same logic in
// its own lines, over the packed bytes of up to 8 nodes per lane: through PairCache its one-node
// instances took 4 to 7 more VGPRs (k3m_matrix<4, 6, 1, false, false, true> 80 -> 84, an occupancy
// step).  It shares subchunk_range.
#pragma once
#include <hip/hip_runtime.h>

#include "dyn_types.hpp"
#include "step_node.hpp"

namespace crane {

// the time range of the pods a wave holds one per lane (live: the lane has a pod), uniform
__device__ __forceinline__ void subchunk_range(bool live, int64_t t, int64_t& cmin, int64_t& cmax) {
    cmin = live ? t : INT64_MAX;
    cmax = live ? t : INT64_MIN;
    wave_minmax64(cmin, cmax);
}

template <class V>
struct PairCache {
    int64_t lo = INT64_MAX, hi = INT64_MIN;  // v0 holds on [lo, hi); empty: nothing is covered
    int64_t bp = INT64_MAX;                  // the step inside the sub-chunk, INT64_MAX = none
    bool multi = false;                      // further steps behind bp inside the sub-chunk
    V v0{}, v1{};                            // the values at cmin and from bp on

    __device__ __forceinline__ bool covers(int64_t cmin, int64_t cmax) const { return cmin >= lo && cmax < hi; }

    template <int PD, int PR, class Eval>
    __device__ __forceinline__ void refresh(const NodeRec<PD, PR>& r, int64_t cmin, int64_t cmax, const Eval& eval) {
        bracket<PD, PR>(r, cmin, lo, hi);
        v0 = eval(cmin, r);
        bp = INT64_MAX;
        multi = false;
        if (hi <= cmax) {
            int64_t lo2, hi2;
            bracket<PD, PR>(r, hi, lo2, hi2);
            bp = hi;
            v1 = eval(hi, r);
            multi = hi2 <= cmax;
        }
    }

    // the value for a pod at time t of the sub-chunk (rec: the node's record, read when multi)
    template <int PD, int PR, class Eval>
    __device__ __forceinline__ V at(int64_t t, const NodeRec<PD, PR>* rec, const Eval& eval) const {
        if (multi) {
            const NodeRec<PD, PR> r = *rec;
            return eval(t, r);
        }
        return t >= bp ? v1 : v0;
    }
};

}  // namespace crane
