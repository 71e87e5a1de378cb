// node_rec.hpp — a node's pod-invariant record (NodeRec) from its parsed
// annotations, shared by the node pass K1 (kernels.hip) and the scatter update
// of changed nodes (update.hip), so both compute it with the same instructions.
//
// Numerics follow /root/reference/pkg/plugins/dynamic/stats.go bit for bit:
// fp64 in the reference's operation order with no FMA contraction (the build
// uses -ffp-contract=off), Go's float64->int conversion and saturating expiry
// sums.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dyn_types.hpp"

namespace crane {

// Go int(float64) on amd64 (CVTTSD2SQ): NaN and out-of-range -> INT64_MIN.
// Used by stats.go:135 (int(score/weight)) and plugins.go:91 (int(hv*10)).
//
// The conversion, the wrapping int64 subtraction after it (plugins.go:91) and the clamp
// (NormalizeScore, utils.go:58-68) are stated in five places, each behind other kernels; a change
// to one is a change to all (tests/test_value_edges_gpu.py drives each with NaN, +-Inf and huge
// inputs against the oracle):
//  1. go_int here: the penalty int(hv * 10) of rec_hot_annotation and rec_hot_counts, i.e. of
//     every NodeRec (K1 in kernels.hip, the streamed K1, the scatter update in update.hip), and
//     the conversion item 3 calls.
//  2. score_of_sum (step_node.hpp): the base int(s / wsum) with a one-instruction path for
//     |q| < 2^31 beside the full conversion, then base - pen wrapping and the clamp.  Through
//     score_at it is the score of the per-pair kernel and the answer tables (matrix.hip), the
//     step path (step.hip, k1stream_body.hpp), topk.hip and select.hip.
//  3. greedy_base, pen_of_sum and final_score (greedy_dev.hpp): base and penalty of the sequential greedy kernels
//     (greedy.hip, greedy_times.hip), the penalty recomputed from the window counts after every
//     placement and, at per-pod times, after every count or expiry that passed.
//  4. RunIter::next (merge.hip): base - 10 v in plain int64, no wrap — valid because M1 raises
//     its flag for any base below INT64_MIN + 2^40 (int(NaN), overflow) and crane_dyn_greedy
//     then runs the sequential kernel instead.
//  5. On the host, go_seconds_trunc (engine.hip) and seconds_trunc (bindings.hpp):
//     int64(d.Seconds()) of binding.go:85, the same range test.
__device__ __forceinline__ int64_t go_int(double x) {
    if (!(x >= -9223372036854775808.0 && x < 9223372036854775808.0)) return INT64_MIN;
    return (int64_t)x;
}

__device__ __forceinline__ int64_t sat_add(int64_t a, int64_t b) {
    int64_t r;
    const bool o = __builtin_add_overflow(a, b, &r);
    return o ? (b > 0 ? INT64_MAX : INT64_MIN) : r;  // (selects: no branch around a caller's loads)
}

// The delta form of K2 keeps its anchor's counts (bz) beside its adjustments (bc, the buckets K1
// reads): the node's window-rank counts from both, in place (rows past n_win read as 0).
__device__ __forceinline__ void bucket_anchor_counts(const uint32_t (&bz)[kMaxWin], uint32_t (&bc)[kMaxWin]) {
#pragma unroll
    for (int b = 0; b < kMaxWin; ++b) bc[b] = bz[b] + bc[b] - (b + 1 < kMaxWin ? bc[b + 1] : 0u);
}

// Predicate and priority parts of the record from the metric rows the policy reads
// (pt / pv: predicate k's (ts, value); qt / qv: priority k's), then e_fail.
template <int PD, int PR>
__device__ __forceinline__ void rec_metrics(const DevPolicy& pol, const int64_t (&pt)[PD], const double (&pv)[PD],
                                            const int64_t (&qt)[PR], const double (&qv)[PR], NodeRec<PD, PR>& r) {
#pragma unroll
    for (int k = 0; k < PD; ++k) {
        int64_t e = kTsInvalid;
        if (k < pol.npd) {
            const int64_t t = pt[k];
            const double u = pv[k];
            const double lim = pol.pred_limit[k];
            // isOverLoad (stats.go:94-112): usable (stats.go:51-76), limit != 0, u > limit
            const bool over = t != kTsInvalid && !(u < 0.0) && lim != 0.0 && u > lim;
            if (over) e = sat_add(t, pol.pred_dur[k]);
        }
        r.e_pred[k] = e;
    }
#pragma unroll
    for (int k = 0; k < PR; ++k) {
        int64_t e = kTsInvalid;
        double term = 0.0;
        if (k < pol.npr) {
            const int64_t t = qt[k];
            const double u = qv[k];
            if (t != kTsInvalid && !(u < 0.0)) {
                e = sat_add(t, pol.prio_dur[k]);
                // getScore (stats.go:89): (1. - usage) * Weight * float64(MaxNodeScore)
                term = (1.0 - u) * pol.prio_w[k];
                term = term * 100.0;
            }
        }
        r.e_prio[k] = e;
        r.t[k] = term;
    }
}

// Predicate k's expiry alone from its metric row (t, u): the e_pred[k] of rec_metrics, the same
// expressions, for a pass that needs no record (the filter diagnosis, diagnose.hip).
__device__ __forceinline__ int64_t pred_expiry(const DevPolicy& pol, int k, int64_t t, double u) {
    const double lim = pol.pred_limit[k];
    // isOverLoad (stats.go:94-112): usable (stats.go:51-76), limit != 0, u > limit
    const bool over = t != kTsInvalid && !(u < 0.0) && lim != 0.0 && u > lim;
    return over ? sat_add(t, pol.pred_dur[k]) : kTsInvalid;
}

// Hot-value part from the node_hot_value annotation (getNodeHotValue, stats.go:152-166:
// no extra active period; an unusable or negative value counts as 0).
template <int PD, int PR>
__device__ __forceinline__ void rec_hot_annotation(double h, int64_t t, NodeRec<PD, PR>& r) {
    r.pen = go_int(h * 10.0);
    r.e_hv = (t != kTsInvalid && !(h < 0.0)) ? sat_add(t, kHotActiveNs) : kTsInvalid;
}

// Hot-value part of the record from the node's K2 window-rank buckets bc[r]
// (annotateNodeHotValue, node.go:113-121: value += count / p.Count, Go int division;
// window w counts the bindings of buckets >= its cutoff rank): one running suffix sum.
// cnt_out / hvc_out (null: not kept): the per-window counts and the value.
template <int PD, int PR, int NW = 0>
__device__ __forceinline__ void rec_hot_counts(const DevPolicy& pol, const uint32_t (&bc)[kMaxWin], int64_t N, int64_t n,
                                               uint32_t* __restrict__ cnt_out, double* __restrict__ hvc_out,
                                               int64_t hv_ts_counts, NodeRec<PD, PR>& r) {
    int64_t v = 0;
    uint64_t suf = 0;
#pragma unroll
    for (int k = kMaxWin - 1; k >= 0; --k) {
        if (k >= (NW ? NW : pol.n_win)) continue;  // (NW: the policy's window count, static)
        // (the rank's words read before any branch or store: one wait for the three)
        const int w = pol.win_of_rank[k];
        const uint32_t dm = pol.win_div_m[k];
        const int32_t dsh = pol.win_div_sh[k];
        suf += bc[k];
        const uint32_t q = div_magic((uint32_t)suf, dm, dsh);
        if (cnt_out) cnt_out[(int64_t)w * N + n] = (uint32_t)suf;
        // Go int division (truncates toward 0): exact multiply-high division when the
        // count fits 32 bits and hotValue.count is in [1, 2^32)
        if (dm != 0 && suf <= 0xFFFFFFFFull)
            v += (int64_t)q;
        else
            v += (int64_t)suf / pol.win_count[w];
    }
    // the plugin re-reads it via ParseFloat (exact) and rejects negatives (stats.go:71-73)
    const double h = (double)v;
    if (hvc_out) hvc_out[n] = h;  // kept for node passes after the buckets are consumed
    r.pen = go_int(h * 10.0);
    r.e_hv = v >= 0 ? sat_add(hv_ts_counts, kHotActiveNs) : kTsInvalid;
}

// The Filter rejects iff now < e_fail = max over the predicates' expiries.
template <int PD, int PR>
__device__ __forceinline__ void rec_fail(NodeRec<PD, PR>& r) {
    int64_t e_fail = kTsInvalid;
#pragma unroll
    for (int k = 0; k < PD; ++k) e_fail = max(e_fail, r.e_pred[k]);
    r.e_fail = e_fail;
}

}  // namespace crane
