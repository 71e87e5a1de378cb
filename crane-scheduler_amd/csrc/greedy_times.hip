// greedy_times.hip — sequential greedy where pod p is scored at its own now[p]
// (crane_dyn_greedy_times): what the reference does with a queue of pods, time.Now() per pod.
//
// The state at pod 0 is crane_dyn_greedy's at now[0] (K2 counts, K1 records, greedy_prep).
// Between two pods three things move with time, each turned into work of the first pod that
// sees it:
//   * an annotation goes stale (stats.go:42-48): a node's base score or feasibility changes at
//     one of its expiries e, for the first pod with !(now_p < e)        -> a record event
//   * a log binding leaves window w (binding.go:85-91): counted at pod p iff
//     ts > unix_p - int64(tr_w.Seconds()); unix_p never decreases, so it leaves at most once,
//     at the first pod where the test fails                             -> a log event (w)
//   * a placement of this batch leaves window w: placements are made in time order and a
//     window's length is constant, so each window keeps one head index into chosen[]
// G3 ev_pass (count, then fill after ev_scan): the events as a CSR by pod, a counting sort.
//    One thread per node (its expiries) and per binding slot (its windows); the pod comes from a
//    binary search over the pod times.  The order inside a pod's group is whatever the fill's
//    atomic cursors gave and nothing depends on it: decrements commute and a touched node's
//    leaf is recomputed from its final counts.
// G4 greedy_run_times: one workgroup over greedy_dev.hpp's tree, descent and re-reduction,
//    the code greedy_run calls, with the counts and base[] reached through WgAccess; before each
//    descent wave 0 advances the window heads, applies the pod's event group 64 events per round
//    and, for every node touched, recomputes base (greedy_base, as greedy_prep), feasibility and
//    the leaf at now[p] and re-reduces its ancestors.  A node not touched keeps a base computed
//    at an earlier time, valid because none of its expiries lies in between.  chosen[p] is
//    stored per pod: a later pod's window head reads it.
//
// The counts are decremented with atomics (two lanes of a round can hit one node).  The kernel is
// one workgroup, so workgroup scope is the whole of it: its atomics, and its other accesses to
// the counts and to the base[] and chosen[] entries it wrote itself, are relaxed workgroup-scope
// atomic operations: coherent per location for the workgroup, on the one compute unit's L1 and
// its XCD's L2 where the atomics execute, and their loads still hit L1 as plain loads do.
//
// A pod with nothing to do before its descent (no event group, no window head due) pays one bit
// test: per 64-pod chunk one mask of the pods with work, rebuilt after each such pod; the window
// heads live in LDS so that the hot loop's scalar registers stay the descent's and the commit's.
#include <hip/hip_runtime.h>

#include "dyn_types.hpp"
#include "greedy_dev.hpp"
#include "kernels.hpp"
#include "wave.hpp"

namespace crane {

constexpr uint32_t kEvRecord = 15;  // event kind: no count changes, the record's answers do (else: the window)
constexpr int kEvThreads = 256;
constexpr size_t kGreedyTimesState = 2 * kMaxWin * sizeof(int64_t);  // LDS behind the tree: the windows' heads

__device__ __forceinline__ uint32_t ev_pack(int64_t node, uint32_t kind) { return (uint32_t)node | (kind << 24); }

// first pod p with !(now[p] < e)
__device__ __forceinline__ int64_t first_pod_at(const int64_t* __restrict__ now, int64_t P, int64_t e) {
    int64_t lo = 0, hi = P;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (now[mid] < e) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// first pod p at which window (trs) no longer counts a binding stamped ts
__device__ __forceinline__ int64_t first_pod_without(const int64_t* __restrict__ unixs, int64_t P, int64_t ts,
                                                     int64_t trs) {
    int64_t lo = 0, hi = P;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (ts > unixs[mid] - trs) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// Thread i < N: node i's expiries inside (now[0], now[P-1]].  Thread N + b: binding slot b, per
// window counted at pod 0 and not at pod P-1.  FILL = false counts the events per pod into
// cur[p]; FILL = true (cur[p] = the group's start, ev_scan) writes them.  P >= 2.
template <int PD, int PR, bool FILL>
__global__ __launch_bounds__(kEvThreads) void ev_pass(const NodeRec<PD, PR>* __restrict__ rec, int64_t N,
                                                      const int32_t* __restrict__ bnode,
                                                      const int64_t* __restrict__ bts, int64_t B,
                                                      GreedyTimesArgs ta, const int64_t* __restrict__ now,
                                                      const int64_t* __restrict__ unixs, int64_t P,
                                                      unsigned long long* __restrict__ cur,
                                                      uint32_t* __restrict__ ev, int64_t E) {
    const int64_t i = (int64_t)blockIdx.x * kEvThreads + threadIdx.x;
    if (i >= N + B) return;
    auto emit = [&](int64_t p, int64_t node, uint32_t kind) {
        if (p <= 0 || p >= P) return;  // (never: the callers' range tests put p in [1, P))
        const unsigned long long at = atomicAdd(&cur[p], 1ull);
        if (FILL && (int64_t)at < E) ev[at] = ev_pack(node, kind);
    };
    if (i < N) {
        const NodeRec<PD, PR>& r = rec[i];
        const int64_t t0 = now[0], t1 = now[P - 1];
        const int64_t ef = r.e_fail;
        if (t0 < ef && !(t1 < ef)) emit(first_pod_at(now, P, ef), i, kEvRecord);
        if (!ta.g.noprio) {
#pragma unroll
            for (int k = 0; k < PR; ++k) {
                const int64_t e = r.e_prio[k];
                if (t0 < e && !(t1 < e)) emit(first_pod_at(now, P, e), i, kEvRecord);
            }
        }
        return;
    }
    const int64_t b = i - N;
    const int32_t nd = bnode[b];
    if (nd < 0 || (int64_t)nd >= N) return;  // an empty slot of the heap's log, a node of another shard
    const int64_t ts = bts[b];
    const int64_t u0 = unixs[0], u1 = unixs[P - 1];
    for (int w = 0; w < ta.g.n_win; ++w) {
        const int64_t trs = ta.trs[w];
        if (ts > u0 - trs && !(ts > u1 - trs)) emit(first_pod_without(unixs, P, ts, trs), nd, (uint32_t)w);
    }
}

// off[0..P] = exclusive prefix sums of c[0..P), c[p] = off[p] (the fill's cursors).  One workgroup.
constexpr int kScanThreads = 1024;
__global__ __launch_bounds__(kScanThreads) void ev_scan(unsigned long long* __restrict__ c, int64_t P,
                                                        int64_t* __restrict__ off) {
    __shared__ unsigned long long part[kScanThreads];
    const int64_t per = (P + kScanThreads - 1) / kScanThreads;
    const int64_t lo = min(P, (int64_t)threadIdx.x * per), hi = min(P, lo + per);
    unsigned long long s = 0;
    for (int64_t p = lo; p < hi; ++p) s += c[p];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int d = 1; d < kScanThreads; d <<= 1) {  // inclusive scan of the threads' sums
        const unsigned long long add = (int)threadIdx.x >= d ? part[threadIdx.x - d] : 0ull;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    unsigned long long run = part[threadIdx.x] - s;
    for (int64_t p = lo; p < hi; ++p) {
        const unsigned long long k = c[p];
        c[p] = run;
        off[p] = (int64_t)run;
        run += k;
    }
    if (threadIdx.x == kScanThreads - 1) off[P] = (int64_t)part[kScanThreads - 1];
}

// ---- the workgroup-scope accesses beside WgAccess's loads and stores (greedy_dev.hpp)
__device__ __forceinline__ void dec_wg(uint32_t* p) {
    (void)__hip_atomic_fetch_sub(p, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// this wave's vector memory operations so far are done (stores and atomics count in vmcnt)
__device__ __forceinline__ void vm_done() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

template <int PD, int PR, int NLEV>
__global__ __launch_bounds__(256) void greedy_run_times(const NodeRec<PD, PR>* __restrict__ rec, int64_t N,
                                                        uint8_t* leaf_g, int64_t* base, uint32_t* cnt,
                                                        GreedyTimesArgs ta, int64_t P,
                                                        const int64_t* __restrict__ now,
                                                        const int64_t* __restrict__ unixs,
                                                        const uint8_t* __restrict__ flags, int64_t* chosen,
                                                        const int64_t* __restrict__ ev_off,
                                                        const uint32_t* __restrict__ ev, int32_t leaves_in_lds) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const GreedyArgs& a = ta.g;
    Tree t;
    const int64_t state_off = tree_layout<NLEV>(t, smem, N, leaves_in_lds);
    uint8_t* leaf = leaves_in_lds ? smem : leaf_g;
    tree_load_build<NLEV, WgAccess>(t, leaf, leaf_g, N, base, cnt, a.n_win, P, chosen);
    if (wave != 0) return;

    // The lanes' nodes (node < 0: none) had a count or an expiry pass: base, feasibility and leaf
    // at nowp from the record and the counts as they are now, then the ancestors of every leaf
    // that changed.  Two lanes may hold one node: they store the same bytes.
    auto refresh = [&](int32_t node, int64_t nowp) {
        bool changed = false;
        if (node >= 0) {
            const NodeRec<PD, PR>& r = rec[node];
            const int64_t b = greedy_base(r, nowp, a);
            const bool feasible = !(nowp < r.e_fail);
            int64_t v = 0;
#pragma unroll
            for (int w = 0; w < kMaxWin; ++w) {
                if (w >= a.n_win) break;
                v += win_quot(WgAccess::ld(&cnt[(int64_t)w * N + node]), a.win_count[w]);
            }
            const uint8_t nl = greedy_leaf(b, pen_of_sum(v), feasible);
            changed = nl != leaf[node];
            WgAccess::st(&base[node], b);  // (the commit reads it)
            leaf[node] = nl;
        }
        vm_done();
        __builtin_amdgcn_wave_barrier();
        uint64_t m = ballot64(changed);
        while (m) {  // at most 64 rounds
            const int j = __builtin_ctzll(m);
            m &= m - 1;
            tree_rereduce<NLEV>(t, leaf, (int64_t)__builtin_amdgcn_readlane(node, j), lane);
        }
    };

    // per window that counts a binding stamped "now" (win_inc): head = the first placement of this
    // batch it still counts, due = the second from which it no longer does, unix[head] + trs
    // (head <= p and trs > 0: a head at the current pod is never due).  Others: never due.
    // Both live in LDS behind the tree (kGreedyTimesState bytes): only pods with work touch them,
    // and the hot loop's scalar registers stay the descent's and the commit's.
    int64_t* const head = reinterpret_cast<int64_t*>(smem + state_off);
    int64_t* const due = head + kMaxWin;
    int64_t next_due = INT64_MAX;
    {
        const int64_t u0 = unixs[0];
#pragma unroll
        for (int w = 0; w < kMaxWin; ++w) {
            const int64_t d = w < a.n_win && a.win_inc[w] ? u0 + ta.trs[w] : INT64_MAX;
            if (lane == 0) {
                head[w] = 0;
                due[w] = d;
            }
            next_due = min(next_due, d);
        }
    }
    for (int64_t p0 = 0; p0 < P; p0 += 64) {
        const int64_t pl = p0 + lane;
        const bool in = pl < P;
        // DaemonSet pods bypass Filter (plugins.go:41-43): one bit per pod of this chunk
        const uint64_t dsmask = ballot64(in && flags && (flags[pl] & 1u));
        // the chunk's times and event groups, one pod per lane; one bit per pod with work before
        // its descent: an event group, or a window with its head due
        const int64_t nowv = in ? now[pl] : 0, unixv = in ? unixs[pl] : 0;
        const int64_t ev0 = in ? ev_off[pl] : 0, ev1 = in ? ev_off[pl + 1] : 0;
        uint64_t work = ballot64(in && (ev0 < ev1 || unixv >= next_due));
        const int np = (int)min((int64_t)64, P - p0);
        for (int q = 0; q < np; ++q) {
            const int64_t p = p0 + q;
            if ((work >> q) & 1) {
                const int64_t nowp = readlane64(nowv, q), unixp = readlane64(unixv, q);
                const int64_t e1 = readlane64(ev1, q);
                // ---- 1. - 3. rounds of at most 64 count changes each, then the touched nodes'
                // leaves: first the placements of this batch leaving a window (window by window,
                // from its head on), then the pod's event group.  Every head round moves a head
                // on by >= 1 (<= p), every event round takes 64 events.
                for (int64_t i0 = readlane64(ev0, q);;) {
                    // the first window whose head placement it no longer counts at this pod
                    int sw = -1;
                    int64_t sh = 0, slim = 0;
                    for (int w = a.n_win - 1; w >= 0; --w) {
                        if (readfirstlane64(due[w]) <= unixp) {
                            sw = w;
                            sh = readfirstlane64(head[w]);
                            slim = unixp - ta.trs[w];
                        }
                    }
                    int32_t node = -1;
                    if (sw >= 0) {
                        vm_done();  // (the commits' stores of chosen[])
                        const int64_t h = sh + lane;
                        const bool out = h < p && unixs[h] <= slim;  // a prefix of the lanes: times never decrease
                        if (out) {
                            node = (int32_t)WgAccess::ld(&chosen[h]);
                            if (node >= 0) dec_wg(&cnt[(int64_t)sw * N + node]);
                        }
                        const int64_t nh = sh + __builtin_popcountll(ballot64(out));  // in (sh, p]
                        if (lane == 0) {
                            head[sw] = nh;
                            due[sw] = unixs[nh] + (unixp - slim);
                        }
                        __builtin_amdgcn_wave_barrier();
                    } else if (i0 < e1) {
                        const int64_t i = i0 + lane;
                        if (i < e1) {
                            const uint32_t e = ev[i];
                            node = (int32_t)(e & 0xFFFFFFu);
                            const uint32_t kind = e >> 24;
                            if (kind < (uint32_t)kMaxWin) dec_wg(&cnt[(int64_t)kind * N + node]);
                        }
                        i0 += 64;
                    } else {
                        break;
                    }
                    vm_done();
                    refresh(node, nowp);
                }
                next_due = INT64_MAX;
                for (int w = 0; w < a.n_win; ++w) next_due = min(next_due, readfirstlane64(due[w]));
                work = ballot64(in && (ev0 < ev1 || unixv >= next_due));  // (the later pods' bits)
            }
            // ---- 4. descent, then the commit: Binding{Node: idx, Timestamp: unix_p}
            const int64_t idx = tree_descend<NLEV>(t, leaf, (dsmask >> q) & 1, lane);
            if (idx < 0) {
                if (lane == 0) WgAccess::st(&chosen[p], idx);
                continue;
            }
            if (lane == 0) {
                // one round trip: counts and base load together, counts stored back
                uint32_t c[kMaxWin];
#pragma unroll
                for (int w = 0; w < kMaxWin; ++w)
                    if (w < a.n_win) c[w] = WgAccess::ld(&cnt[(int64_t)w * N + idx]);
                const int64_t b = WgAccess::ld(&base[idx]);
                int64_t v = 0;
#pragma unroll
                for (int w = 0; w < kMaxWin; ++w) {
                    if (w >= a.n_win) break;
                    c[w] += a.win_inc[w] ? 1u : 0u;
                    WgAccess::st(&cnt[(int64_t)w * N + idx], c[w]);
                    v += win_quot(c[w], a.win_count[w]);
                }
                const uint8_t old = leaf[idx];
                leaf[idx] = (uint8_t)(final_score(b, pen_of_sum(v)) | (old & 0x80));
                WgAccess::st(&chosen[p], idx);  // (a later pod's step 1 reads it)
            }
            // LDS instructions of one wave execute in order; a global leaf store is waited for
            if (!leaves_in_lds) vm_done();
            __builtin_amdgcn_wave_barrier();
            tree_rereduce<NLEV>(t, leaf, idx, lane);
        }
    }
}

template <int PD, int PR>
static hipError_t launch_events_t(const void* rec, int64_t N, const int32_t* bnode, const int64_t* bts, int64_t B,
                                  const GreedyTimesArgs& a, const int64_t* now, const int64_t* unixs, int64_t P,
                                  unsigned long long* cur, uint32_t* ev, int64_t E, bool fill, hipStream_t st) {
    const int64_t n = N + B;
    if (n <= 0 || P < 2) return hipSuccess;
    const dim3 grid((unsigned)((n + kEvThreads - 1) / kEvThreads));
    const NodeRec<PD, PR>* r = static_cast<const NodeRec<PD, PR>*>(rec);
    if (fill)
        return klaunch("greedy_ev_fill", ev_pass<PD, PR, true>, grid, dim3(kEvThreads), 0, st, r, N, bnode, bts, B, a,
                       now, unixs, P, cur, ev, E);
    return klaunch("greedy_ev_count", ev_pass<PD, PR, false>, grid, dim3(kEvThreads), 0, st, r, N, bnode, bts, B, a,
                   now, unixs, P, cur, ev, E);
}

hipError_t launch_greedy_events(int shape, const void* rec, int64_t N, const int32_t* bnode, const int64_t* bts,
                                int64_t B, const GreedyTimesArgs& a, const int64_t* now, const int64_t* unixs,
                                int64_t P, unsigned long long* cur, uint32_t* ev, int64_t E, bool fill,
                                hipStream_t st) {
    if (N + B > 0x7FFFFFFFll * kEvThreads) return hipErrorInvalidValue;
    return with_shape(shape, [&](auto pd, auto pr) {
        return launch_events_t<pd(), pr()>(rec, N, bnode, bts, B, a, now, unixs, P, cur, ev, E, fill, st);
    });
}

hipError_t launch_greedy_events_scan(unsigned long long* cur, int64_t P, int64_t* off, hipStream_t st) {
    return klaunch("greedy_ev_scan", ev_scan, dim3(1), dim3(kScanThreads), 0, st, cur, P, off);
}

hipError_t launch_greedy_times(int shape, const void* rec, int64_t N, uint32_t* cnt, const GreedyTimesArgs& a,
                               int64_t* base, uint8_t* leaf, int64_t P, const int64_t* now, const int64_t* unixs,
                               const uint8_t* flags, int64_t* chosen, const int64_t* ev_off, const uint32_t* ev,
                               hipStream_t st) {
    if (N <= 0 || N > kGreedyMaxNodes || P <= 0) return hipErrorInvalidValue;
    const GreedyTreeShape ts = greedy_tree_shape(N, kGreedyTimesState);
    return with_shape(shape, [&](auto pd, auto pr) {
        return with_levels(ts.nlev, [&](auto L) {
            return launch_greedy_run<greedy_run_times<pd(), pr(), L()>>(
                "greedy_run_times", ts.lds_bytes, st, static_cast<const NodeRec<pd(), pr()>*>(rec), N, leaf, base, cnt,
                a, P, now, unixs, flags, chosen, ev_off, ev, (int32_t)ts.in_lds);
        });
    });
}

}  // namespace crane
