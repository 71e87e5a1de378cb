// step_node.hpp — per-node part of the K3 step path (step.hip), shared by the
// stand-alone step-table kernel K3a and the fused node pass K1+K3a
// (kernels.hip), which builds the step tables straight from the NodeRec it
// has just computed in registers.
//
// A node's packed key (score << 24 | 0xFFFFFF - node, -1 = the pod may not go
// there) is a step function of the pod's `now`; over a batch whose times lie
// in [tmin, tmax] only the node's expiries inside (tmin, tmax] can change it.
// A node with none is "flat": its key is the same for every pod of a kind and
// only enters the workgroup's flat max.  Otherwise the node appends a Step1
// (one step) or VRec (more) record to its kind's compact list.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "dyn_types.hpp"
#include "kernels.hpp"
#include "wave.hpp"

namespace crane {

// Producer block of workgroup b of nb: workgroups are dispatched round-robin
// over the 8 XCDs, so XCD x gets a contiguous run of blocks (its L2 then
// shares the cache lines of neighbouring blocks' inputs).  A bijection on [0, nb).
__device__ __forceinline__ int64_t xcd_block(int64_t b, int64_t nb) {
    const int64_t x = b & 7, q = b >> 3, per = nb >> 3, rem = nb & 7;
    return x * per + (x < rem ? x : rem) + q;
}

// Exact clamped Score of (pod at time t, node) — the literal int64 restatement
// of stats.go:114-138 + plugins.go:91-93, the semantics of K3's eval_pair and
// score_exact (kernels.hip).
template <int PD, int PR>
// winv: 1 / wsum when |wsum| is a power of two (the default policy's weights sum to 2.0), else
// 0: the reciprocal is then exact and s * winv the same correctly rounded quotient as s / wsum,
// one multiply instead of the division sequence (a uniform branch).
__device__ __forceinline__ int32_t score_at(int64_t t, const NodeRec<PD, PR>& r, double wsum, int32_t noprio,
                                          double winv = 0.0);

// The score from the ordered sum s of the active priority terms and the active hot-value
// penalty pen (0 when inactive): score_at's tail, shared with the streamed count pass.
__device__ __forceinline__ int32_t score_of_sum(double s, int64_t pen, double wsum, int32_t noprio, double winv) {
    int64_t base = 0;
    if (!noprio) {
        const double q = winv != 0.0 ? s * winv : s / wsum;  // stats.go:135 int(score / weight), Go CVTTSD2SQ
        // |q| < 2^31 (every realistic score): one v_cvt_i32_f64 truncates toward zero exactly as
        // the 64-bit conversion does; otherwise the full CVTTSD2SQ restatement (NaN, overflow)
        if (__builtin_fabs(q) < 2147483648.0) base = (int64_t)(int32_t)q;
        else base = (q >= -9223372036854775808.0 && q < 9223372036854775808.0) ? (int64_t)q : INT64_MIN;
    }
    const int64_t f = (int64_t)((uint64_t)base - (uint64_t)pen);  // plugins.go:91, wraps like Go
    return (int32_t)(f < 0 ? 0 : (f > 100 ? 100 : f));            // NormalizeScore (utils.go:58-68)
}

template <int PD, int PR>
__device__ __forceinline__ int32_t score_at(int64_t t, const NodeRec<PD, PR>& r, double wsum, int32_t noprio,
                                          double winv) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < PR; ++k)
        if (t < r.e_prio[k]) s += r.t[k];  // stats.go:124-133, policy order
    return score_of_sum(s, t < r.e_hv ? r.pen : 0, wsum, noprio, winv);
}

// Filter (plugins.go:41-43, 55-66) + packed key for pod kind T (0: Filter applies, 1: DaemonSet)
template <int PD, int PR>
__device__ __forceinline__ int32_t key_of(int T, int64_t t, int32_t score, const NodeRec<PD, PR>& r, int64_t n) {
    return (T == 1 || !(t < r.e_fail)) ? pack_key(score, n) : -1;
}

// Batch time range [tmin, tmax] from K3p's per-tile partials, in two parts so
// a kernel can issue the loads early and reduce after its own loads:
// batch_range_load (per-thread partials), batch_range_reduce (every thread of
// the workgroup gets the result; sm*: >= BS/64 LDS entries; has a barrier).
template <int BS>
__device__ __forceinline__ void batch_range_load(const int64_t* __restrict__ tile_mm, int32_t ntiles, int64_t& mn,
                                                 int64_t& mx) {
    mn = INT64_MAX;
    mx = INT64_MIN;
    for (int i = threadIdx.x; i < ntiles; i += BS) {
        const int64_t* ts = tile_mm + kTileStat * i;
        mn = min(mn, min(ts[0], ts[2]));
        mx = max(mx, max(ts[1], ts[3]));
    }
}
template <int BS>
__device__ __forceinline__ void batch_range_reduce(int64_t mn, int64_t mx, int64_t* smn, int64_t* smx, int64_t& tmin,
                                                   int64_t& tmax) {
    wave_minmax64(mn, mx);
    if ((threadIdx.x & 63) == 0) {
        smn[threadIdx.x >> 6] = mn;
        smx[threadIdx.x >> 6] = mx;
    }
    __syncthreads();
    tmin = smn[0];
    tmax = smx[0];
#pragma unroll
    for (int i = 1; i < BS / 64; ++i) {
        tmin = min(tmin, smn[i]);
        tmax = max(tmax, smx[i]);
    }
}
template <int BS>
__device__ __forceinline__ void batch_range(const int64_t* __restrict__ tile_mm, int32_t ntiles, int64_t* smn,
                                            int64_t* smx, int64_t& tmin, int64_t& tmax) {
    int64_t mn, mx;
    batch_range_load<BS>(tile_mm, ntiles, mn, mx);
    batch_range_reduce<BS>(mn, mx, smn, smx, tmin, tmax);
}

// [lo, hi): the node's results are constant for every time in it (lo = latest expiry
// <= t, hi = earliest expiry > t; the comparisons are now < expiry)
template <int PD, int PR>
__device__ __forceinline__ void bracket(const NodeRec<PD, PR>& r, int64_t t, int64_t& lo, int64_t& hi) {
    lo = INT64_MIN;
    hi = INT64_MAX;
    auto upd = [&](int64_t e) {
        if (e <= t) lo = max(lo, e);
        else hi = min(hi, e);
    };
#pragma unroll
    for (int k = 0; k < PD; ++k) upd(r.e_pred[k]);
#pragma unroll
    for (int k = 0; k < PR; ++k) upd(r.e_prio[k]);
    upd(r.e_hv);
}

// exclusive workgroup scan (BT threads): wave scans + a scan of the wave totals
template <int BT = 256>
__device__ __forceinline__ uint32_t wg_excl_scan_u32(uint32_t v, uint32_t* part) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t x = wave_scan_add(v);  // (DPP lane moves: every thread of the workgroup calls this)
    if (lane == 63) part[w] = x;
    __syncthreads();
    uint32_t pre = 0;
#pragma unroll
    for (int i = 0; i < BT / 64; ++i) pre += i < w ? part[i] : 0u;
    __syncthreads();
    return pre + x - v;
}

// Per node and pod kind: the flat key (-1 if stepped or never feasible) and,
// for a stepped node, its slots in the workgroup's spans of the kind's lists.
// Phase 1 (step_count) only classifies — cheap and register-light, so it can
// run inside the node pass; phase 2 (step_emit) rebuilds the record of a
// stepped node after the workgroup has reserved its list spans.
//
// A stepped node's key is piecewise constant over the batch: key_0 before its
// first in-range expiry c_0, key_j on [c_{j-1}, c_j), key_m from c_{m-1} on.
// It is published as pieces: two one-step records for the half-lines —
// (bp c_0: key_0 before, -1 after) and (bp c_{m-1}: -1 before, key_m after),
// or one (bp c_0: key_0 before, key_1 after) when m = 1 — and m - 1 middle
// pieces [c_j, c_{j+1}) with their keys.  The max over a node's pieces covering
// a time is its key then (a piece covers nothing outside its interval, -1).
struct StepSlots {
    int32_t flat0 = -1, flat1 = -1;
    int32_t slot0 = -1, slot1 = -1;    // >= 0: stepped (first one-step record slot)
    int32_t mslot0 = 0, mslot1 = 0;    // first middle-piece slot
    bool multi0 = false, multi1 = false;
};

// Workgroup-shared counters of the step epilogue.
struct StepShared {
    int32_t lc[2][2];   // per kind: [one-step records, middle pieces]
    int32_t fm[2][16];  // per-wave flat maxima (<= 1024 threads)
    int32_t pn[2];      // per kind: elementary pieces after step_pieces, -1 = raw pieces
};
// the block's flat maximum of kind T from the per-wave maxima (after the barrier behind their stores)
template <int BS>
__device__ __forceinline__ int32_t block_flat_max(const StepShared& sh, int T) {
    int32_t m = sh.fm[T][0];
#pragma unroll
    for (int i = 1; i < BS / 64; ++i) m = max(m, sh.fm[T][i]);
    return m;
}

// The classifier every producer shares.  StepRange: a node's expiries inside the batch range
// (tmin, tmax] for one pod kind — the only ones that can change its key over the batch — folded
// one at a time: their number (with repeats), minimum and maximum.  A node with one distinct
// in-range expiry (a predicate's expiry equals its metric's priority expiry when both use one
// metric) is one record; otherwise two half-line records and cnt - 1 middle-piece slots are
// reserved (repeated expiries give empty pieces, harmless: they cover no time).
struct StepRange {
    int cnt = 0;
    int64_t mn = INT64_MAX, mx = INT64_MIN;
    __device__ __forceinline__ void add(int64_t e, int64_t tmin, int64_t tmax) {
        const bool in = e > tmin && e <= tmax;
        cnt += in;
        mn = in ? min(mn, e) : mn;
        mx = in ? max(mx, e) : mx;
    }
    __device__ __forceinline__ bool multi() const { return cnt > 0 && mn != mx; }  // (cnt == 0: mn > mx)
    // what the node takes of its kind's spans: one-step records | middle pieces << 16
    __device__ __forceinline__ uint32_t word() const {
        return (cnt ? (multi() ? 2u : 1u) : 0u) | (multi() ? (uint32_t)(cnt - 1) << 16 : 0u);
    }
};
// Both kinds' ranges g[T] from the expiries they share (both: the priorities', the hot value's):
// kind 0 also steps at e_fail (DaemonSet pods, kind 1, bypass the Filter); a lane without a node
// (!valid) has none.  Sets o's flat keys — the node's key at tmin (score s0) when nothing steps,
// else -1 — and multi flags.
__device__ __forceinline__ void step_classify(const StepRange& both, int64_t e_fail, bool valid, int32_t s0, int64_t n,
                                              int64_t tmin, int64_t tmax, StepRange (&g)[2], StepSlots& o) {
    g[0] = g[1] = both;
    g[0].add(e_fail, tmin, tmax);
    if (!valid) g[0].cnt = g[1].cnt = 0;
    o.multi0 = g[0].multi();
    o.multi1 = g[1].multi();
    o.flat0 = valid && g[0].cnt == 0 && !(tmin < e_fail) ? pack_key(s0, n) : -1;  // key_of at tmin
    o.flat1 = valid && g[1].cnt == 0 ? pack_key(s0, n) : -1;
}
// The node's slots from at[T]: its kind's span base + the exclusive prefix of the word()s before it
// (packed like word(): the sums stay under 2^16).
__device__ __forceinline__ void step_slots(const StepRange (&g)[2], uint32_t at0, uint32_t at1, StepSlots& o) {
    o.slot0 = g[0].cnt ? (int32_t)(at0 & 0xFFFF) : -1;
    o.mslot0 = g[0].multi() ? (int32_t)(at0 >> 16) : 0;
    o.slot1 = g[1].cnt ? (int32_t)(at1 & 0xFFFF) : -1;
    o.mslot1 = g[1].multi() ? (int32_t)(at1 >> 16) : 0;
}
// the expiries both kinds share, of a record
template <int PD, int PR>
__device__ __forceinline__ StepRange step_range(const NodeRec<PD, PR>& r, int64_t tmin, int64_t tmax) {
    StepRange sh;
#pragma unroll
    for (int k = 0; k < PR; ++k) sh.add(r.e_prio[k], tmin, tmax);
    sh.add(r.e_hv, tmin, tmax);
    return sh;
}

// Phase 1 (the stand-alone K3a, threads with a node): spans taken with one LDS atomic per counter.
template <int PD, int PR>
__device__ __forceinline__ void step_count(const NodeRec<PD, PR>& r, int64_t n, int64_t tmin, int64_t tmax,
                                           double wsum, int32_t noprio, StepShared& sh, StepSlots& o) {
    StepRange g[2];
    step_classify(step_range(r, tmin, tmax), r.e_fail, true, score_at<PD, PR>(tmin, r, wsum, noprio), n, tmin, tmax,
                  g, o);
    uint32_t at[2] = {0, 0};
#pragma unroll
    for (int T = 0; T < 2; ++T) {
        const uint32_t w = g[T].word();
        if (w) at[T] = (uint32_t)atomicAdd(&sh.lc[T][0], (int32_t)(w & 0xFFFF));
        if (w >> 16) at[T] |= (uint32_t)atomicAdd(&sh.lc[T][1], (int32_t)(w >> 16)) << 16;
    }
    step_slots(g, at[0], at[1], o);
}

// Phase 2, one (node, kind): the node's one-step records go to the workgroup's
// staging (S1Out) (LDS, or st.stage when the block's records exceed the
// LDS staging; step_sort_publish writes them out sorted), its middle pieces
// straight to st.mid.
// Where a block's one-step records go: its LDS staging (lds, kind stride kl) or, when the block
// holds more of a kind than that takes (g, workgroup-uniform), st.stage (glb, stride kg).  Two
// stores with known address spaces: one store through a pointer selected between LDS and global
// is a flat store, which goes down the vector memory path even for LDS (round 5: the streamed
// pass's emit 2.6 -> 1.3 us per workgroup without them).
struct S1Out {
    Step1* lds;
    Step1* glb;
    bool g;
    int64_t kl, kg;
    __device__ __forceinline__ void put(int T, int32_t i, const Step1& v) const {
        if (g) glb[T * kg + i] = v;
        else lds[T * kl + i] = v;
    }
};

template <int PD, int PR>
__device__ __forceinline__ void step_emit_one(const NodeRec<PD, PR>& r, int64_t n, int T, int32_t slot,
                                              int32_t mslot, bool multi, int64_t tmin, int64_t tmax, double wsum,
                                              int32_t noprio, const StepTables& st, int64_t blk, const S1Out& s1o,
                                              double winv = 0.0) {
    constexpr int NB = PR + 2;
    int64_t c[NB];
#pragma unroll
    for (int k = 0; k < PR; ++k) c[k] = r.e_prio[k];
    c[PR] = r.e_hv;
    c[PR + 1] = T == 0 ? r.e_fail : INT64_MIN;  // DaemonSet pods bypass the Filter
    int cnt = 0;
    int64_t mn = INT64_MAX;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        const bool in = c[j] > tmin && c[j] <= tmax;
        c[j] = in ? c[j] : INT64_MAX;
        cnt += in;
        mn = min(mn, c[j]);
    }
    auto key = [&](int64_t t) {  // key_of for the run-time kind, at the first instant of a step
        const int32_t f = score_at<PD, PR>(t, r, wsum, noprio, winv);
        return (T == 1 || !(t < r.e_fail)) ? pack_key(f, n) : -1;
    };
    const int32_t k0 = key(tmin);
    if (!multi) {
        Step1 v;
        v.bp = mn;
        v.k0 = k0;
        v.k1 = key(mn);
        s1o.put(T, slot, v);
        return;
    }
#pragma unroll
    for (int i = 0; i < NB; ++i)  // odd-even transposition sort (static indices)
#pragma unroll
        for (int j = i & 1; j + 1 < NB; j += 2) {
            const int64_t x = c[j], y = c[j + 1];
            c[j] = min(x, y);
            c[j + 1] = max(x, y);
        }
    Mid* md = st.mid + (int64_t)T * st.mpad + blk * st.mstride + mslot;
    int32_t kprev = k0;
    int64_t last = c[0];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        if (j >= cnt) continue;
        const int32_t kj = key(c[j]);  // the key from c[j] on
        if (j + 1 < cnt) {
            Mid p;
            p.s = c[j];
            p.e = c[j + 1];
            p.key = kj;
            p.pad = 0;
            md[j] = p;
        }
        last = c[j];
        kprev = kj;
    }
    Step1 a, b;
    a.bp = c[0];
    a.k0 = k0;
    a.k1 = -1;
    b.bp = last;
    b.k0 = -1;
    b.k1 = kprev;
    s1o.put(T, slot, a);
    s1o.put(T, slot + 1, b);
}

// Phase 2 for every kind of a node (the stand-alone K3a).
template <int PD, int PR>
__device__ __forceinline__ void step_emit(const NodeRec<PD, PR>& r, int64_t n, int64_t tmin, int64_t tmax,
                                          double wsum, int32_t noprio, const StepSlots& o,
                                          const StepTables& st, int64_t blk, const S1Out& s1o,
                                          double winv = 0.0) {
    if (o.slot0 >= 0)
        step_emit_one<PD, PR>(r, n, 0, o.slot0, o.mslot0, o.multi0, tmin, tmax, wsum, noprio, st, blk, s1o, winv);
    if (o.slot1 >= 0)
        step_emit_one<PD, PR>(r, n, 1, o.slot1, o.mslot1, o.multi1, tmin, tmax, wsum, noprio, st, blk, s1o, winv);
}

// K1's form of step_count + stepped-record staging + the emit's work queue, called by every
// thread of the workgroup (valid: the thread has a node): the per-lane counts are prefix-summed
// across the wave (DPP) and one lane takes the wave's spans with one LDS atomic per
// counter, instead of a chain of per-lane returning atomics.  Slots are assigned in lane
// order (any order is a valid one: K3s takes maxima).  keep: records written out (the
// record slot is the thread's; every item queued), else the stepped records are staged in
// lrec[0, CAP) and a node past the staging builds its own (self_emit; its queue items
// are marked ~0u).
// Work item q[i]: owner thread | kind << 12 | multi << 13 | slot << 14 | rs << 24, its first
// middle-piece slot in qm[i] (rs: the node's record slot in the LDS staging, < 256; slot < 1024).
template <int PD, int PR, int CAP>
__device__ __forceinline__ void step_count_queue(const NodeRec<PD, PR>& r, bool valid, int64_t n, int64_t tmin,
                                                 int64_t tmax, double wsum, double winv, int32_t noprio,
                                                 bool keep, StepShared& sh, int32_t* nrec, int32_t* nq,
                                                 uint32_t* q, int32_t* qm, NodeRec<PD, PR>* lrec, StepSlots& o,
                                                 bool& self_emit) {
    StepRange g[2];
    step_classify(step_range(r, tmin, tmax), r.e_fail, valid, score_at<PD, PR>(tmin, r, wsum, noprio, winv), n, tmin,
                  tmax, g, o);
    const int cnt0 = g[0].cnt, cnt1 = g[1].cnt;
    // per lane: one-step records | middle pieces << 16 per kind; stepped | queue items << 16
    const uint32_t w0 = g[0].word(), w1 = g[1].word();
    const uint32_t w2 = ((cnt0 | cnt1) ? 1u : 0u) | (((cnt0 ? 1u : 0u) + (cnt1 ? 1u : 0u)) << 16);
    // exclusive prefixes and the wave's totals (lane 63's inclusive prefix)
    uint32_t e0 = wave_scan_add(w0);
    const uint32_t t0 = __builtin_amdgcn_readlane(e0, 63);
    e0 -= w0;
    uint32_t e1 = wave_scan_add(w1);
    const uint32_t t1 = __builtin_amdgcn_readlane(e1, 63);
    e1 -= w1;
    uint32_t e2 = wave_scan_add(w2);
    const uint32_t t2 = __builtin_amdgcn_readlane(e2, 63);
    e2 -= w2;
    int32_t b[6] = {0, 0, 0, 0, 0, 0};
    if ((threadIdx.x & 63) == 63) {
        if (t0) {
            b[0] = atomicAdd(&sh.lc[0][0], (int32_t)(t0 & 0xFFFF));
            b[1] = atomicAdd(&sh.lc[0][1], (int32_t)(t0 >> 16));
        }
        if (t1) {
            b[2] = atomicAdd(&sh.lc[1][0], (int32_t)(t1 & 0xFFFF));
            b[3] = atomicAdd(&sh.lc[1][1], (int32_t)(t1 >> 16));
        }
        if (t2) {
            b[4] = atomicAdd(nrec, (int32_t)(t2 & 0xFFFF));
            b[5] = atomicAdd(nq, (int32_t)(t2 >> 16));
        }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) b[k] = __builtin_amdgcn_readlane(b[k], 63);
    step_slots(g, ((uint32_t)b[0] | (uint32_t)b[1] << 16) + e0, ((uint32_t)b[2] | (uint32_t)b[3] << 16) + e1, o);
    self_emit = false;
    if (cnt0 | cnt1) {
        int rs = b[4] + (int32_t)(e2 & 0xFFFF);
        bool staged = true;
        if (keep) rs = threadIdx.x;
        else if (rs < CAP) lrec[rs] = r;
        else staged = false;
        int qi = b[5] + (int32_t)(e2 >> 16);
        if (cnt0) {
            q[qi] = staged ? threadIdx.x | ((uint32_t)o.multi0 << 13) | ((uint32_t)o.slot0 << 14) | ((uint32_t)rs << 24)
                           : ~0u;
            qm[qi] = o.mslot0;
            ++qi;
        }
        if (cnt1) {
            q[qi] = staged ? threadIdx.x | (1u << 12) | ((uint32_t)o.multi1 << 13) | ((uint32_t)o.slot1 << 14) |
                                 ((uint32_t)rs << 24)
                           : ~0u;
            qm[qi] = o.mslot1;
        }
        self_emit = !staged;
    }
}

// step_publish's stores, after the barrier behind sh.fm (the streamed pass folds that barrier into
// its own and calls them itself): thread T < 2 kind T's flat maximum, thread 2 + L counter L
// (kind L >> 1: one-step records, L & 1 = 0, or middle pieces) = cnt(L)
template <int BS, class Cnt>
__device__ __forceinline__ void step_publish_store(const StepShared& sh, const StepTables& st, int64_t blk, Cnt cnt) {
    if (threadIdx.x < 2) st.flat[blk * 2 + threadIdx.x] = block_flat_max<BS>(sh, threadIdx.x);
    else if (threadIdx.x < 6) st.cnt[blk * 4 + threadIdx.x - 2] = cnt((int)threadIdx.x - 2);
}
// Workgroup epilogue: the workgroup's flat-key maxima and record counts go to
// its own slots (producer block blk) of the step tables (plain stores, no global atomics).  Every
// thread calls it (barrier); sh.lc must have been zeroed before step_count.
template <int BS>
__device__ __forceinline__ void step_publish(const StepSlots& o, StepShared& sh, const StepTables& st, int64_t blk) {
    auto wmax = [&](int T, int32_t m) {
        m = wave_max(m);
        if ((threadIdx.x & 63) == 0) sh.fm[T][threadIdx.x >> 6] = m;
    };
    wmax(0, o.flat0);
    wmax(1, o.flat1);
    __syncthreads();
    step_publish_store<BS>(sh, st, blk, [&](int L) { return sh.lc[L >> 1][L & 1]; });
}

// number of the n sorted records at a[] with bp <= t (upper bound)
__device__ __forceinline__ int32_t count_le(const Step1* a, int32_t n, int64_t t) {
    int32_t lo = 0, hi = n;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (a[mid].bp <= t) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// Prefix max of k1 (pm1) / suffix max of k0 (sm0) over a block's sorted one-step records, after
// the barrier behind the sort: wave T scans kind T (a one-wave workgroup both in turn) in chunks of
// 64 consecutive records, one per lane, with a carry.  L: the sorted records are srt[2][CAP] in
// LDS and the maxima are also kept there, in pmL[2][CAP] and behind it smL[2][CAP], for the tile
// rows; else the records are read from st.single.
template <int BS, int CAP, bool L>
__device__ __forceinline__ void step_scan_maxima(const Step1* srt, int32_t* pmL, const StepShared& sh,
                                                 const StepTables& st, int64_t blk) {
    const int n0 = sh.lc[0][0], n1 = sh.lc[1][0];
    int32_t* smL = pmL + 2 * CAP;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int T = w; T < 2; T += (BS >= 128 ? 2 : 1)) {
        const int n = T ? n1 : n0;
        const int64_t base = s1_at(st, T, blk);
        const Step1* a = L ? srt + T * CAP : st.single + base;
        int32_t carry = -1;
        for (int c0 = 0; c0 < n; c0 += 64) {
            const int i = c0 + lane;
            const int32_t v = max(wave_scan_max(i < n ? a[i].k1 : -1), carry);
            if (i < n) {
                st.pm1[base + i] = v;
                if (L) pmL[T * CAP + i] = v;
            }
            carry = __builtin_amdgcn_readlane(v, 63);
        }
        // suffix maxima: lane l takes index c0 + 63 - l, so a prefix in lane order
        carry = -1;
        for (int c0 = (n - 1) & ~63; c0 >= 0 && n > 0; c0 -= 64) {
            const int i = c0 + 63 - lane;
            const int32_t v = max(wave_scan_max(i < n ? a[i].k0 : -1), carry);
            if (i < n) {
                st.sm0[base + i] = v;
                if (L) smL[T * CAP + i] = v;
            }
            carry = __builtin_amdgcn_readlane(v, 63);
        }
    }
}

// After every Step1 record of the workgroup is in s1l (and a barrier): per pod kind,
// the records sorted by step time bp go to the workgroup's region of st.single, with
// pm1[i] = max of k1 over sorted records 0..i (the keys after their steps) and
// sm0[i] = max of k0 over records i..n-1 (the keys before their steps).  For a pod
// tile's range [lo, hi] of a kind, the records stepping inside are [jl, jh) (jl = those
// with bp <= lo, jh = those with bp <= hi) and every pod of it takes every other
// record's key from one prefix and one suffix maximum: step_tile_rows writes that
// uniform key (with the flat maximum) and [jl, jh) per tile into st.rows (when set),
// so K3s starts from them; without rows K3s searches the records itself.
// s1l: LDS staging [2][CAP] records (CAP >= either kind's count), srt: LDS scratch
// [2][CAP]; s1l is reused for the maxima.  Every thread calls it (barriers); sh.fm
// holds the per-wave flat maxima (step_publish).
template <int BS, int CAP = 2 * BS>
__device__ __forceinline__ void step_sort_publish(Step1* s1l, Step1* srt, const StepShared& sh,
                                                  const StepTables& st, int64_t blk) {
    const int n0 = sh.lc[0][0], n1 = sh.lc[1][0];
    // rank sort (ties by slot): typically a few dozen records per kind
    for (int i = threadIdx.x; i < n0 + n1; i += BS) {
        const int T = i >= n0;
        const int k = T ? i - n0 : i;
        const int n = T ? n1 : n0;
        const Step1* a = s1l + T * CAP;
        const Step1 v = a[k];
        int rank = 0;
        int j = 0;
        for (; j + 8 <= n; j += 8) {  // 8 independent LDS reads in flight
            int64_t b[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) b[u] = a[j + u].bp;
#pragma unroll
            for (int u = 0; u < 8; ++u) rank += (b[u] < v.bp) || (b[u] == v.bp && j + u < k);
        }
        for (; j < n; ++j) {
            const int64_t b = a[j].bp;
            rank += (b < v.bp) || (b == v.bp && j < k);
        }
        srt[T * CAP + rank] = v;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n0 + n1; i += BS) {
        const int T = i >= n0;
        const int k = T ? i - n0 : i;
        st.single[s1_at(st, T, blk) + k] = srt[T * CAP + k];
    }
    step_scan_maxima<BS, CAP, true>(srt, reinterpret_cast<int32_t*>(s1l), sh, st, blk);  // (s1l is free now)
}

// The same for a block whose records exceed the LDS staging: staged in st.stage
// (same indexing as st.single), ranked straight into st.single, maxima into pm1 / sm0.
template <int BS>
__device__ __forceinline__ void step_sort_publish_global(const StepShared& sh, const StepTables& st, int64_t blk) {
    const int n0 = sh.lc[0][0], n1 = sh.lc[1][0];
    for (int i = threadIdx.x; i < n0 + n1; i += BS) {
        const int T = i >= n0;
        const int k = T ? i - n0 : i;
        const int n = T ? n1 : n0;
        const Step1* a = st.stage + s1_at(st, T, blk);
        const Step1 v = a[k];
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const int64_t b = a[j].bp;
            rank += (b < v.bp) || (b == v.bp && j < k);
        }
        st.single[s1_at(st, T, blk) + rank] = v;
    }
    __syncthreads();
    step_scan_maxima<BS, 0, false>(nullptr, nullptr, sh, st, blk);
}

// ---- middle pieces -> disjoint elementary pieces (per block and kind, after the emit)
// A kind's raw middle pieces [s, e) (every multi-step node's: they overlap across nodes)
// are cut at every piece end into disjoint intervals, each carrying the max key of the
// pieces covering it; intervals no feasible piece covers are dropped.  At any time the
// max over the raw pieces containing it is the key of the one elementary piece containing
// it, so a pod tile needs only the pieces its time range overlaps — a contiguous range
// [pl, ph) of the sorted list (step_tile_rows writes it to st.prow; one covering the whole
// range goes into the row's uniform key) — instead of every piece of the block once per
// tile (config 4: ~32 pieces per kind and block, 98 tiles).  The list replaces the raw
// one in st.mid (and its count in st.cnt).  Kinds with more than the scratch holds, or too
// little work to pay for it (pieces x tiles < st.piece_work), stay raw: their row range is
// all pieces.
// LDS scratch per kind (pc pieces at most): sorted breakpoints bs[2pc] (i64), unsorted
// bu[2pc] (i64: s, e of piece k at 2k, 2k + 1), maxima vm[2pc] (of the interval from each
// sorted breakpoint to the next), compacted positions ix[2pc], raw keys rk[pc] (i32):
// 52 * pc bytes.
struct PieceScr {
    unsigned char* p;
    int32_t pc;  // pieces per kind the scratch holds (0: never decompose)
    __device__ int64_t* bs(int T) const { return reinterpret_cast<int64_t*>(p + (int64_t)T * 52 * pc); }
    __device__ int64_t* bu(int T) const { return reinterpret_cast<int64_t*>(p + (int64_t)T * 52 * pc + 16 * pc); }
    __device__ int32_t* vm(int T) const { return reinterpret_cast<int32_t*>(p + (int64_t)T * 52 * pc + 32 * pc); }
    __device__ int32_t* ix(int T) const { return reinterpret_cast<int32_t*>(p + (int64_t)T * 52 * pc + 40 * pc); }
    __device__ int32_t* rk(int T) const { return reinterpret_cast<int32_t*>(p + (int64_t)T * 52 * pc + 48 * pc); }
    static constexpr int bytes_per_piece = 2 * 52;  // both kinds
};
// Every thread calls it (barriers when a kind is decomposed); sh.lc final and the emit's
// pieces in st.mid (a barrier after the emit).  Sets sh.pn (read after the next barrier).
template <int BS>
__device__ __forceinline__ void step_pieces(StepShared& sh, const StepTables& st, int64_t blk, const PieceScr& ps) {
    const int32_t nm0 = sh.lc[0][1], nm1 = sh.lc[1][1];
    auto dec = [&](int32_t nm) {
        return st.prow && nm >= 2 && nm <= ps.pc && (int64_t)nm * st.ntiles >= st.piece_work;
    };
    const bool d0 = dec(nm0), d1 = dec(nm1);
    if (!d0 && !d1) {  // (workgroup-uniform)
        if (threadIdx.x < 2) sh.pn[threadIdx.x] = -1;
        return;
    }
    const int32_t a0 = d0 ? nm0 : 0, a1 = d1 ? nm1 : 0;  // pieces taken per kind
    // A: the raw pieces into LDS
    for (int i = threadIdx.x; i < a0 + a1; i += BS) {
        const int T = i >= a0, k = T ? i - a0 : i;
        const Mid m = st.mid[(int64_t)T * st.mpad + blk * st.mstride + k];
        ps.bu(T)[2 * k] = m.s;
        ps.bu(T)[2 * k + 1] = m.e;
        ps.rk(T)[k] = m.key;
    }
    __syncthreads();
    // B: every breakpoint v (s or e of a piece) in one pass over its kind's pieces: its
    // rank among the breakpoints (ties by index: its position in the sorted order) and the
    // max key of the feasible pieces covering [v, next breakpoint), i.e. with s <= v < e
    // (broadcast LDS reads, no atomics: equal breakpoints get equal maxima)
    for (int i = threadIdx.x; i < 2 * (a0 + a1); i += BS) {
        const int T = i >= 2 * a0, j = T ? i - 2 * a0 : i, n = T ? a1 : a0;
        const int64_t* b = ps.bu(T);
        const int32_t* rk = ps.rk(T);
        const int64_t v = b[j];
        int32_t r = 0, m = -1;
        for (int k = 0; k < n; ++k) {
            const int64_t s = b[2 * k], e = b[2 * k + 1];
            r += (s < v) || (s == v && 2 * k < j);
            r += (e < v) || (e == v && 2 * k + 1 < j);
            if (s <= v && v < e) m = max(m, rk[k]);
        }
        ps.bs(T)[r] = v;
        ps.vm(T)[r] = m;
    }
    __syncthreads();
    // D: wave T compacts kind T's non-empty covered intervals (in order) and publishes them
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int T = w; T < 2; T += (BS >= 128 ? 2 : 1)) {  // wave T compacts kind T (one wave: both)
        const int32_t n = 2 * (T ? a1 : a0);
        if ((T ? d1 : d0)) {
            const int64_t* bs = ps.bs(T);
            const int32_t* vm = ps.vm(T);
            Mid* out = st.mid + (int64_t)T * st.mpad + blk * st.mstride;
            uint32_t carry = 0;
            for (int32_t c0 = 0; c0 < n - 1; c0 += 64) {
                const int32_t j = c0 + lane;
                const bool f = j < n - 1 && bs[j] < bs[j + 1] && vm[j] >= 0;
                const uint32_t inc = wave_scan_add(f ? 1u : 0u);
                if (f) {
                    const int32_t pos = (int32_t)(carry + inc - 1);
                    ps.ix(T)[pos] = j;
                    Mid m;
                    m.s = bs[j];
                    m.e = bs[j + 1];
                    m.key = vm[j];
                    m.pad = 0;
                    out[pos] = m;
                }
                carry += __builtin_amdgcn_readlane(inc, 63);
            }
            if (lane == 0) {
                sh.pn[T] = (int32_t)carry;
                st.cnt[blk * 4 + 2 * T + 1] = (int32_t)carry;
            }
        } else if (lane == 0) {
            sh.pn[T] = -1;
        }
    }
}

// The tile rows (st.rows set): per pod tile t, the block's uniform key per kind and
// the range [jl, jh) of its sorted one-step records stepping inside the tile's range
// (after step_sort_publish: srt sorted, s1l holding the prefix / suffix maxima), and
// (st.prow set) the range [pl, ph) of its middle pieces overlapping it (step_pieces).
// pre: this thread's first item's bound (tile_prefetch, loaded early).  Every thread
// calls it (barrier).
__device__ __forceinline__ void tile_prefetch(const StepTables& st, int64_t* pre) {
    const int x = threadIdx.x;  // item x: tile x / 4, kind (x / 2) % 2, lo / hi
    *pre = (x >> 2) < st.ntiles ? st.tiles[kTileStat * (x >> 2) + ((x >> 1) & 1) * 2 + (x & 1)] : 0;
}
// G: the block's records went through st.stage (step_sort_publish_global): the
// searches read st.single / pm1 / sm0 instead of the LDS copies.
template <int BS, int CAP = 2 * BS, bool G = false>
__device__ __forceinline__ void step_tile_rows(const Step1* s1l, const Step1* srt, const StepShared& sh,
                                               const StepTables& st, int64_t blk, const int64_t* pre,
                                               const PieceScr& ps) {
    const int n0 = sh.lc[0][0], n1 = sh.lc[1][0];
    const int32_t* pmL = reinterpret_cast<const int32_t*>(s1l);
    const int32_t* smL = pmL + 2 * CAP;
    __syncthreads();
    const int32_t fl[2] = {block_flat_max<BS>(sh, 0), block_flat_max<BS>(sh, 1)};
    // item i: tile i / 4, kind (i / 2) % 2, bound i % 2 (lo, hi): one LDS search each, the
    // four items of a tile on adjacent lanes combine by shuffles
    for (int i0 = 0; i0 < 4 * st.ntiles; i0 += BS) {
        const int i = i0 + threadIdx.x;
        const int t = i >> 2, T = (i >> 1) & 1, hi_b = i & 1;
        const int n = T ? n1 : n0;
        const int32_t pn = sh.pn[T];
        int32_t c = 0, u = -1, pc = 0;
        int64_t v = 0;
        if (t < st.ntiles) {
            v = i0 == 0 ? *pre : st.tiles[kTileStat * t + 2 * T + hi_b];
            if (G) {
                const int64_t base = s1_at(st, T, blk);
                c = count_le(st.single + base, n, v);
                if (!hi_b && c > 0) u = st.pm1[base + c - 1];
                if (hi_b && c < n) u = st.sm0[base + c];
            } else {
                c = count_le(srt + T * CAP, n, v);
                if (!hi_b && c > 0) u = pmL[T * CAP + c - 1];  // records stepped by lo: keys after
                if (hi_b && c < n) u = smL[T * CAP + c];       // records stepping after hi: keys before
            }
            // middle pieces: elementary ones ending by lo (pl) / starting by hi (ph); raw: all
            if (!st.prow) {
            } else if (pn >= 0) {
                const int64_t* bs = ps.bs(T);
                const int32_t* ix = ps.ix(T);
                int32_t lo = 0, hi = pn;
                while (lo < hi) {
                    const int32_t mid = (lo + hi) >> 1;
                    if (bs[ix[mid] + (hi_b ? 0 : 1)] <= v) lo = mid + 1;
                    else hi = mid;
                }
                pc = lo;
            } else {
                pc = hi_b ? sh.lc[T][1] : 0;
            }
        }
        const int32_t co = quad_xor1(c), uo = quad_xor1(u);
        const int32_t jl = hi_b ? co : c, jh = hi_b ? c : co;
        int32_t ukey = -1, pp = 0;
        if (st.prow) {  // (uniform)
            const int32_t pco = quad_xor1(pc);
            const int64_t vo = (int64_t)(((uint64_t)(uint32_t)quad_xor1((int32_t)((uint64_t)v >> 32)) << 32) |
                                         (uint32_t)quad_xor1((int32_t)(uint32_t)v));
            int32_t pl = hi_b ? pco : pc;
            const int32_t ph = hi_b ? pc : pco;
            if (pn >= 0 && ph - pl == 1 && t < st.ntiles) {  // one elementary piece: uniform if it covers [lo, hi]
                const int64_t lo_v = hi_b ? vo : v, hi_v = hi_b ? v : vo;
                const int32_t j = ps.ix(T)[pl];
                if (ps.bs(T)[j] <= lo_v && ps.bs(T)[j + 1] > hi_v) {
                    ukey = ps.vm(T)[j];
                    pl = ph;
                }
            }
            pp = pl < ph ? (pl | (ph << 16)) : 0;
        }
        // a kind without pods here (lo = INT64_MAX, hi = INT64_MIN) gives jl = n > jh = 0
        const int32_t um = jl > jh ? -1 : max(max(fl[T], ukey), max(u, uo)), jp = jl > jh ? 0 : (jl | (jh << 16));
        const int32_t um1 = quad_down2(um), jp1 = quad_down2(jp);
        const int32_t pp1 = st.prow ? quad_down2(pp) : 0;
        if ((i & 3) == 0 && t < st.ntiles) {
            st.rows[(int64_t)t * st.nblk + blk] = make_int4(um, um1, jp, jp1);
            if (st.prow) st.prow[(int64_t)t * st.nblk + blk] = make_int2(pp, pp1);
        }
    }
}

// The producers' epilogue, after every one-step record and middle piece of the block is out (and
// a barrier): sort + publish (stamp 6), and with st.rows the elementary pieces and the tile rows.
// g1 (workgroup-uniform): the block's one-step records went through st.stage, else they are in
// s1l[2][CAP].  pre: this thread's first tile bound when the caller loaded it early
// (tile_prefetch), null: loaded here, behind the sort.  ps: the LDS the caller can lend the pieces.
// Every thread of the BS calls it (barriers).
template <int BS, int CAP>
__device__ __forceinline__ void step_epilogue(bool g1, Step1* s1l, Step1* srt, StepShared& sh, const StepTables& st,
                                              int64_t blk, const int64_t* pre, const PieceScr& ps,
                                              unsigned long long* trace, int64_t wg) {
    if (g1) step_sort_publish_global<BS>(sh, st, blk);
    else step_sort_publish<BS, CAP>(s1l, srt, sh, st, blk);
    CRANE_TSTAMP(trace, wg, 6);
    if (!st.rows) return;
    int64_t late = 0;
    if (!pre) {
        tile_prefetch(st, &late);
        pre = &late;
    }
    step_pieces<BS>(sh, st, blk, ps);
    if (g1) step_tile_rows<BS, CAP, true>(s1l, srt, sh, st, blk, pre, ps);
    else step_tile_rows<BS, CAP, false>(s1l, srt, sh, st, blk, pre, ps);
}

// ---- step_sort_publish + step_tile_rows for a block of few one-step records, in registers.
// At 3 % stepped nodes a 256-node block holds about ten records per kind: the sorted LDS copy, the
// scans and the searches above are then three barriers and five LDS round trips for a few hundred
// bytes.  None of it is needed, not even the sort.  With a kind's n <= 32 records one per lane,
//   a record's sorted position is #{records before it} (before: smaller bp, ties by slot), its
//   pm1 the max of k1 over those and itself, its sm0 the max of k0 over the others;
//   a tile bound v has count_le = #{bp <= v}, pmL[c - 1] = max{k1 : bp <= v} (the bound lo) and
//   smL[c] = max{k0 : bp > v} (hi)
// — one question asked of every record j, broadcast from lane j (readlane: no LDS, no scan, no
// search): is it under this lane's threshold w (bp < w, or bp == w and j < tl)?  Lanes 0-31 ask
// it as record `lane` (w its bp, tl its slot), lanes 32-63 as tile item lane - 32 of a round of 32
// (tile x >> 1, bound x & 1; w the bound, tl past every slot), in the same loop: small_scan.
// Wave-local, no barrier.  The words written are step_sort_publish's and step_tile_rows' without
// st.prow, bit for bit (keys are >= -1).
struct SmallScan {
    int32_t cnt;  // records under the threshold
    int32_t a;    // max k1 over them
    int32_t b;    // max k0 over the others
};
// r: lane j < n holds record j of the kind (n wave-uniform)
__device__ __forceinline__ SmallScan small_scan(const Step1& r, int n, int64_t w, int tl) {
    SmallScan s{0, -1, -1};
    for (int j = 0; j < n; ++j) {
        const int64_t bj = readlane64(r.bp, j);
        const int32_t k0j = __builtin_amdgcn_readlane(r.k0, j), k1j = __builtin_amdgcn_readlane(r.k1, j);
        const bool under = bj < w || (bj == w && j < tl);
        s.cnt += under;
        s.a = max(s.a, under ? k1j : -1);
        s.b = max(s.b, under ? -1 : k0j);
    }
    return s;
}
// the bound of item lane `lane` (32-63) of the round whose first tile is t0, for kind T; other lanes 0
__device__ __forceinline__ int64_t small_tile_bound(const StepTables& st, int T, int t0, int lane) {
    const int t = t0 + ((lane - 32) >> 1);
    return lane >= 32 && t < st.ntiles ? st.tiles[kTileStat * t + 2 * T + (lane & 1)] : 0;
}
// the records' part of a scan with w = the lane's own bp, tl = lane: step_sort_publish's stores
__device__ __forceinline__ void small_records_store(int T, int n, const Step1& r, const SmallScan& s,
                                                    const StepTables& st, int64_t blk) {
    const int lane = threadIdx.x & 63;
    if (lane < n) {
        const int64_t at = s1_at(st, T, blk) + s.cnt;
        st.single[at] = r;
        st.pm1[at] = max(s.a, r.k1);  // sorted positions <= its own
        st.sm0[at] = s.b;             // ... >= its own (itself is not under its threshold)
    }
}
// the items' part of a scan with w = small_tile_bound, tl = 64: the bounds of a tile (adjacent
// lanes) combine as step_tile_rows' do, and the kind stores its own two words of the tile's row
// (kind 0 .x / .z, kind 1 .y / .w: two waves taking a kind each exchange nothing).  fl: the
// block's flat maximum of the kind.  Every lane of the wave calls it (DPP).
__device__ __forceinline__ void small_row_store(int T, int t0, const SmallScan& s, int32_t fl, const StepTables& st,
                                                int64_t blk) {
    const int lane = threadIdx.x & 63, t = t0 + ((lane - 32) >> 1);
    const bool hi_b = lane & 1;
    // lo: records stepped by it, their keys after; hi: records stepping after it, before
    const int32_t c = s.cnt, u = hi_b ? s.b : s.a;
    const int32_t co = quad_xor1(c), uo = quad_xor1(u);
    const int32_t jl = hi_b ? co : c, jh = hi_b ? c : co;
    // a kind without pods here (lo = INT64_MAX, hi = INT64_MIN) gives jl = n > jh = 0
    const int32_t um = jl > jh ? -1 : max(fl, max(u, uo)), jp = jl > jh ? 0 : (jl | (jh << 16));
    if (lane >= 32 && !hi_b && t < st.ntiles) {
        int32_t* row = reinterpret_cast<int32_t*>(st.rows + ((int64_t)t * st.nblk + blk));
        row[T] = um;
        row[2 + T] = jp;
    }
}

}  // namespace crane
