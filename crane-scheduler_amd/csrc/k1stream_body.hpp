// k1stream_body.hpp — the body of the streamed node pass fused with the step tables (K1 for
// large N), shared by its own kernel (k1stream.hip) and the one-launch queue step (step.hip,
// step_one_launch), where it runs beside another batch's K3s and a third's K2 + K3p.
//
// Numerics: the same per-term arithmetic as node_rec.hpp / step_node.hpp (stats.go:89-138,
// plugins.go:39-98 bit for bit, -ffp-contract=off).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "dyn_types.hpp"
#include "kernels.hpp"
#include "node_rec.hpp"
#include "step_node.hpp"

namespace crane {

// The node pass fused with the step tables, without a NodeRec in registers.  Round 4 found what
// holds the fused pass at 0.41 of HBM cold: occupancy, which the 160 B record costs (96 VGPRs,
// five waves per SIMD) — a count pass that folds each row into what classification needs as it
// arrives runs at seven waves and 0.59 on its own — and every way of handing the ~3 % stepped
// nodes' records to a separate emit kernel cost more than it saved.  Here the
// hand-off stays inside the workgroup:
//   A  each lane streams its node's rows and keeps only e_fail, the hot-value penalty and
//      expiry, and per pod kind the in-range expiry count / min / max and the flat key;
//   B  wave prefix sums + one exchange of the waves' totals give every stepped node its
//      one-step / middle-piece slots and its rank among the block's stepped nodes;
//   C  in chunks of kSRec stepped nodes: each stepped lane writes its e_fail / pen / e_hv and
//      slots into an LDS record, the workgroup then gathers the chunk's priority rows from L2
//      (one (node, term) per lane: the lines this workgroup streamed microseconds earlier) and
//      writes e_prio / t with rec_metrics' arithmetic, and the first lanes emit the chunk's
//      (node, kind) items from the LDS records (step_emit_one);
//   D  the fused pass's tail: sort + publish, elementary pieces, tile rows.
// Not with the dedupe-form K2 entries (their per-block counting needs the default pass's LDS).
// step_emit_one's outputs for the stepped nodes of a chunk, spread over the lanes: node j takes
// lanes j * (PR + 2) + q, and lane q handles candidate expiry q (the priorities', the hot
// value's, e_fail) for both pod kinds at once: if it is in the batch range, its rank r in the
// kind's ascending order (with multiplicity, by ranking the candidates in registers), its key
// (one score serves both kinds: the Filter only gates kind 0's), its middle piece
// [c_r, c_{r+1}), and — r = 0 / r = cnt - 1 — the half-line records.  A node's keys are then
// computed side by side instead of one after another (round 5's first form, one lane per item
// walking its expiries in order with the record read from LDS term by term, spent 4.9 us per
// workgroup here: a chain of dependent LDS reads; a lane per (node, kind, candidate) doubled the
// emitting waves for 1 % more time).  The outputs are step_emit_one's, bit for bit.
// K1S_SKIP (cost ablation builds only, tools/gpu_k1_ablate.sh; wrong tables): 1 no emit tasks,
// 2 no tail (sort / pieces / tile rows), 4 no record staging, 8 middle pieces left raw (no
// elementary pieces: the tables stay right, K3s reads every piece), 16 no tile rows
#ifndef K1S_SKIP
#define K1S_SKIP 0
#endif
#ifndef K1S_TAIL1  // the single-wave tail for grids of many rounds (A/B: 0 off)
#define K1S_TAIL1 1
#endif
#ifndef K1S_WAVES  // waves per SIMD the 4x6 form is built for (72 VGPRs: 7; 64: 8)
#define K1S_WAVES 7
#endif
#ifndef K1S_KWARM  // the kernarg lines warmed in the scalar cache while the rows load (A/B: 0 off)
#define K1S_KWARM 1
#endif
#ifndef K1S_FULL  // the instance for a policy of exactly 4 predicates / 6 priorities / 2 windows (A/B: 0 off)
#define K1S_FULL 1
#endif
#ifndef K1S_SREC
#define K1S_SREC 64
#endif
#ifndef K1S_SCAP
#define K1S_SCAP 128
#endif
#ifndef K1S_RTAIL  // the register tail for blocks of few one-step records (A/B: 0 the generic tail always)
#define K1S_RTAIL 1
#endif
#ifndef K1S_SMALL  // kSmallTail (A/B: 16; at most 32)
#define K1S_SMALL 32
#endif
constexpr int kSRec = K1S_SREC;  // stepped records staged per chunk
constexpr int kSCap = K1S_SCAP;  // one-step records per kind staged in LDS (more: st.stage)
// one-step records per kind up to which a block takes the register tail (small_tail): one per
// lane of a half wave (the other half takes the tile bounds), each lane walking all of them
constexpr int kSmallTail = K1S_SMALL;
static_assert(kSmallTail <= 32 && kSmallTail <= kSCap, "one record per lane of a half wave, staged in LDS");

template <int PD, int PR>
__device__ __forceinline__ void emit_task(const NodeRec<PD, PR>& r, int64_t n, int q, const int32_t* dw, int64_t tmin,
                                          int64_t tmax, double wsum, int32_t noprio, const StepTables& st,
                                          int64_t blk, const S1Out& s1o, double winv) {
    constexpr int NB = PR + 2, F = PR + 1;  // candidate F = e_fail: kind 0's only (DaemonSet pods bypass the Filter)
    int64_t c[NB];
#pragma unroll
    for (int k = 0; k < PR; ++k) c[k] = r.e_prio[k];
    c[PR] = r.e_hv;
    c[F] = r.e_fail;
    uint32_t inm = 0;  // kind 0's in-range candidates; kind 1's are inm without F
#pragma unroll
    for (int k = 0; k < NB; ++k) inm |= (c[k] > tmin && c[k] <= tmax) ? 1u << k : 0u;
    if (!((inm >> q) & 1u)) return;  // out of range
    const int cnt0 = __builtin_popcount(inm), cnt1 = __builtin_popcount(inm & ~(1u << F));
    // c[q], its rank in the ascending order of (c, index) and the next one's value, per kind:
    // ranks among NB registers (static indices) instead of a sort
    int64_t cq = c[0];
#pragma unroll
    for (int j = 1; j < NB; ++j) cq = q == j ? c[j] : cq;
    int rk0 = 0;
    bool fb = false;  // e_fail before c[q] (kind 0 only)
    int64_t cn1 = INT64_MAX, cn0;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        const bool in = (inm >> j) & 1u;
        const bool before = in && (c[j] < cq || (c[j] == cq && j < q));
        const bool after = in && (c[j] > cq || (c[j] == cq && j > q));
        rk0 += before;
        if (j == F) {
            fb = before;
            cn0 = after ? min(cn1, c[j]) : cn1;
        } else {
            cn1 = after ? min(cn1, c[j]) : cn1;
        }
    }
    const int rk1 = rk0 - (fb ? 1 : 0);
    // one score per instant serves both kinds (the Filter only gates kind 0's key): score_at with
    // the expiries already in c[] and the terms read side by side (one LDS wait, not one per term)
    double tk[PR];
#pragma unroll
    for (int k = 0; k < PR; ++k) tk[k] = r.t[k];
    double ssum = 0.0;
#pragma unroll
    for (int k = 0; k < PR; ++k) ssum = cq < c[k] ? ssum + tk[k] : ssum;  // stats.go:124-133, policy order
    const int64_t pk = pack_key(score_of_sum(ssum, cq < c[PR] ? r.pen : 0, wsum, noprio, winv), n);
    // the score at tmin: phase A's, kept in the record's slot words (dw[5])
    const int64_t pk0 = pack_key(dw[5], n);
#pragma unroll
    for (int T = 0; T < 2; ++T) {
        const int32_t slot = dw[T ? 2 : 0];
        if (slot < 0 || (T == 1 && q == F)) continue;
        const int rk = T ? rk1 : rk0, cnt = T ? cnt1 : cnt0;
        const int64_t cn = T ? cn1 : cn0;
        const int32_t kq = (int32_t)((T == 1 || !(cq < r.e_fail)) ? pk : -1);    // the key from c_rk on
        const int32_t kt = (int32_t)((T == 1 || !(tmin < r.e_fail)) ? pk0 : -1); // ... before c_0
        const bool multi = ((dw[4] >> T) & 1) != 0;
        if (!multi) {  // one record: before / from the one distinct expiry
            if (rk == 0) {
                Step1 v;
                v.bp = cq;
                v.k0 = kt;
                v.k1 = kq;
                s1o.put(T, slot, v);
            }
            continue;
        }
        if (rk + 1 < cnt) {
            Mid pc;
            pc.s = cq;
            pc.e = cn;
            pc.key = kq;
            pc.pad = 0;
            (st.mid + (int64_t)T * st.mpad + blk * st.mstride + dw[T ? 3 : 1])[rk] = pc;
        }
        if (rk == 0) {
            Step1 x;
            x.bp = cq;
            x.k0 = kt;
            x.k1 = -1;
            s1o.put(T, slot, x);
        }
        if (rk == cnt - 1) {
            Step1 y;
            y.bp = cq;
            y.k0 = -1;
            y.k1 = kq;
            s1o.put(T, slot + 1, y);
        }
    }
}

// the step epilogue after the emit: sort + publish, elementary pieces, tile rows, by the BS
// threads still running (lrec: the staged records' LDS, dead now: the pieces' scratch)
template <int BS, class Rec>
__device__ __forceinline__ void tail(bool g1, Rec* lrec, Step1* s1l, Step1* srt, StepShared& ssh, const K1Step& step,
                                     int64_t blk, unsigned long long* trace, int64_t wg) {
    constexpr int kPc = ((int)(kSRec * sizeof(Rec)) / PieceScr::bytes_per_piece) & ~3;
    const PieceScr ps{reinterpret_cast<unsigned char*>(lrec), (K1S_SKIP & 8) ? 0 : (kPc < 128 ? kPc : 128)};
#if K1S_SKIP & 16
    StepTables st = step.st;
    st.rows = nullptr;
#else
    const StepTables& st = step.st;
#endif
    // (no early tile_prefetch: the first tile bounds load behind the sort)
    step_epilogue<BS, kSCap>(g1, s1l, srt, ssh, st, blk, nullptr, ps, trace, wg);
    CRANE_TSTAMP(trace, wg, 4);
}

// The same epilogue for a block of at most kSmallTail one-step records per kind (n0 / n1, staged in
// s1l) in a step without st.prow, in registers and wave-local (step_node.hpp small_scan): kind T
// on wave T (the caller's waves 2 and 3 have left), or with ONE both kinds in turn on wave 0.
// Lanes 0-31 are the kind's records, lanes 32-63 the bounds of the first 16 tiles (pre: loaded by
// the caller before the emit, small_tail_bounds), so one scan gives the records' positions and
// maxima and the rows; more tiles take further scans.  No barrier: the caller had one after the
// emit; ssh.fm holds the per-wave flat maxima.  Nothing is stored before the last scan of round 0
// (a wait for a later load would wait for the stores too).  Stamp 6 is wave 0's after its records
// went out, 4 its end.
// (small_tail_bounds: the first 16 tiles' bounds of this wave's kind, or with ONE of both kinds)
template <bool ONE>
__device__ __forceinline__ void small_tail_bounds(const StepTables& st, int64_t (&pre)[2]) {
    const int lane = threadIdx.x & 63;
    const int T0 = ONE ? 0 : __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    pre[0] = small_tile_bound(st, T0, 0, lane);
    pre[1] = ONE ? small_tile_bound(st, 1, 0, lane) : 0;
}
template <bool ONE>
__device__ __forceinline__ void small_tail(const Step1* s1l, int32_t n0, int32_t n1, const StepShared& ssh,
                                           const K1Step& step, int64_t blk, const int64_t (&pre)[2], bool rows,
                                           unsigned long long* trace, int64_t wg) {
    constexpr int NK = ONE ? 2 : 1;
    const StepTables& st = step.st;
    const int lane = threadIdx.x & 63;
    const int T0 = ONE ? 0 : __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int tl = lane < 32 ? lane : 64;  // ties: a record by slot, a bound takes every bp <= it
    int32_t n[NK], fl[NK];
    Step1 r[NK];
    SmallScan sc[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int T = T0 + k;
        n[k] = __builtin_amdgcn_readfirstlane(T ? n1 : n0);
        fl[k] = block_flat_max<256>(ssh, T);
        r[k].bp = 0;
        r[k].k0 = r[k].k1 = -1;
        if (lane < n[k]) r[k] = s1l[T * kSCap + lane];
    }
#pragma unroll
    for (int k = 0; k < NK; ++k) sc[k] = small_scan(r[k], n[k], lane < 32 ? r[k].bp : pre[k], tl);
#pragma unroll
    for (int k = 0; k < NK; ++k) small_records_store(T0 + k, n[k], r[k], sc[k], st, blk);
    CRANE_TSTAMP(trace, wg, 6);
    if (rows) {
#pragma unroll
        for (int k = 0; k < NK; ++k) small_row_store(T0 + k, 0, sc[k], fl[k], st, blk);
        for (int t0 = 16; t0 < st.ntiles; t0 += 16) {
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                const SmallScan s = small_scan(r[k], n[k], small_tile_bound(st, T0 + k, t0, lane), 64);
                small_row_store(T0 + k, t0, s, fl[k], st, blk);
            }
        }
    }
    CRANE_TSTAMP(trace, wg, 4);
}

// FULL: the policy has exactly PD predicates, PR priorities and kFullWin hot-value windows (the
// reference's shipped policy at 4 x 6): every per-term loop is static, so the policy words load
// together instead of one scalar load and wait per term under its own uniform branch
constexpr int kFullWin = 2;
// the pass's LDS (one workgroup of 256 lanes): its own kernel holds one statically, the
// one-launch step carves it from the launch's union (step.hip)
template <int PD, int PR>
struct K1Lds {
    // a staged stepped node's record: e_fail, pen, e_hv, e_prio, t (what the emit reads), and in
    // e_pred's first words its slots per kind (slot < 0: none), multi flags and the score at tmin
    alignas(16) NodeRec<PD, PR> lrec[kSRec];
    alignas(16) Step1 s1l[2 * kSCap];  // one-step staging, then pm / sm maxima
    alignas(16) Step1 srt[2 * kSCap];  // sorted copy
    alignas(16) uint32_t xch[5][4];
    StepShared ssh;
    uint8_t rank_lane[256];  // a stepped node's rank in the block -> its lane
};
// wg of nwg: the workgroup's index among the pass's workgroups (its own kernel: the grid's);
// WARM: the bytes of the launch's kernarg segment up to the end of this pass's arguments
template <int PD, int PR, bool FULL, int WARM>
__device__ __forceinline__ void k1_stream_body(const K1Args& a, const K1Step& step, const int64_t wg, const int64_t nwg,
                                               K1Lds<PD, PR>& lds) {
    using Rec = NodeRec<PD, PR>;
    constexpr int BS = 256;
    const int npd = FULL ? PD : a.pol.npd, npr = FULL ? PR : a.pol.npr, nwin = FULL ? kFullWin : a.pol.n_win;
    Rec* const lrec = lds.lrec;
    uint8_t* const rank_lane = lds.rank_lane;
    Step1* const s1l = lds.s1l;
    Step1* const srt = lds.srt;
    uint32_t(*const xch)[4] = lds.xch;
    StepShared& ssh = lds.ssh;
    const DevPolicy& pol = a.pol;
    const int64_t N = a.N;
    const int64_t blk = xcd_block(wg, nwg), first = blk * BS, n = first + threadIdx.x;
    CRANE_TSTAMP(a.trace, wg, 0);
    const int lo = (int)min((int64_t)threadIdx.x, N - 1 - first);  // lane offset, clamped
    // the batch range K3p folded: loaded first, so waiting for it does not wait for the rows
    const int64_t bt0 = step.batch[0], bt1 = step.batch[1];
    // ---- A: stream the rows (every load unconditional, clamped index: all in flight at once)
    int64_t pt[PD], qt[PR];
    double pv[PD], qv[PR];
#pragma unroll
    for (int k = 0; k < PD; ++k) {
        pt[k] = kTsInvalid;
        pv[k] = 0.0;
    }
#pragma unroll
    for (int k = 0; k < PR; ++k) {
        qt[k] = kTsInvalid;
        qv[k] = 0.0;
    }
    if (FULL || pol.n_slots > 0) {  // (FULL: the policy reads metrics)
#pragma unroll
        for (int k = 0; k < PD; ++k) {
            const int64_t row = k < npd ? pol.pred_slot[k] : 0;
            pt[k] = (a.ts + (row * N + first))[lo];
            pv[k] = (a.val + (row * N + first))[lo];
        }
#pragma unroll
        for (int k = 0; k < PR; ++k) {
            const int64_t row = k < npr ? pol.prio_slot[k] : 0;
            qt[k] = (a.ts + (row * N + first))[lo];
            qv[k] = (a.val + (row * N + first))[lo];
        }
    }
    uint32_t bc[kMaxWin];
    double hvl = 0.0;
    int64_t hvt = kTsInvalid;
    if (a.buckets) {
        // (+ the delta form's anchor counts: node_rec.hpp bucket_anchor_counts)
        const uint32_t* __restrict__ base = a.bucket_base ? a.bucket_base : a.buckets;
        uint32_t bz[kMaxWin];
#pragma unroll
        for (int b = 0; b < kMaxWin; ++b) {
            bc[b] = b < nwin ? (a.buckets + first)[(int64_t)b * N + lo] : 0u;
            bz[b] = b < nwin ? (base + first)[(int64_t)b * N + lo] : 0u;
        }
        if (a.bucket_base) bucket_anchor_counts(bz, bc);  // (rows past n_win read as 0)
    } else if (a.hv) {
        hvl = a.hv[first + lo];
        hvt = a.hv_ts ? a.hv_ts[first + lo] : a.hv_ts_counts;
    }
#if K1S_KWARM
    kernarg_warm<WARM>();
#endif
    // the batch range K3p folded, uniform: kept in SGPRs
    const int64_t tmin = readfirstlane64(bt0), tmax = readfirstlane64(bt1);
    if (threadIdx.x < 4) ssh.lc[threadIdx.x >> 1][threadIdx.x & 1] = 0;
    CRANE_TSTAMP(a.trace, wg, 1);
    const bool valid = n < N;
    // isOverLoad per predicate (stats.go:94-112): the Filter rejects iff now < e_fail
    int64_t e_fail = kTsInvalid;
    // (every policy word read unconditionally, the per-term conditions as selects: the scalar
    // loads then issue together instead of one wait per term under its own branch)
#pragma unroll
    for (int k = 0; k < PD; ++k) {
        const double u = pv[k], lim = pol.pred_limit[k];
        const int64_t e = sat_add(pt[k], pol.pred_dur[k]);
        const bool over = k < npd && pt[k] != kTsInvalid && !(u < 0.0) && lim != 0.0 && u > lim;
        e_fail = over ? max(e_fail, e) : e_fail;
    }
    // hot value (getNodeHotValue / the binding-log counts) -> penalty and its expiry
    Rec hr;  // (only pen / e_hv are set and read)
    if (a.buckets) {
        if (valid && !a.buckets_keep) {
#pragma unroll
            for (int b = 0; b < kMaxWin; ++b)  // consumed: leaves the buckets zeroed for the next K2
                if (b < nwin) (a.buckets + first)[(int64_t)b * N + threadIdx.x] = 0;
        }
        rec_hot_counts<PD, PR, FULL ? kFullWin : 0>(pol, bc, N, n, valid ? a.cnt_out : nullptr, valid ? a.hvc_out : nullptr,
                               a.hv_ts_counts, hr);
    } else if (a.hv) {
        rec_hot_annotation<PD, PR>(hvl, hvt, hr);
    } else {
        hr.pen = 0;
        hr.e_hv = kTsInvalid;
    }
    // priorities in policy order: score_at(tmin)'s ordered sum and the in-range expiries both
    // pod kinds share (priorities, hot value); e_fail is kind 0's too (DaemonSet pods bypass)
    double s = 0.0;
    StepRange both;
    // the terms stay in registers (they replace the rows' ts / usage) until a stepped lane has
    // its record slot (after B): no second read of the rows
    int64_t ep[PR];
    double tp[PR];
#pragma unroll
    for (int k = 0; k < PR; ++k) {
        const bool use = k < npr && qt[k] != kTsInvalid && !(qv[k] < 0.0);
        double term = (1.0 - qv[k]) * pol.prio_w[k];  // getScore (stats.go:89), no FMA
        term = term * 100.0;
        const int64_t e = sat_add(qt[k], pol.prio_dur[k]);
        ep[k] = use ? e : kTsInvalid;
        tp[k] = use ? term : 0.0;
        s = tmin < ep[k] ? s + tp[k] : s;  // stats.go:124-133
        both.add(ep[k], tmin, tmax);
    }
    both.add(hr.e_hv, tmin, tmax);
    const int32_t s0 = score_of_sum(s, tmin < hr.e_hv ? hr.pen : 0, step.wsum, step.noprio, step.winv);
    StepRange g[2];
    StepSlots so;
    step_classify(both, e_fail, valid, s0, n, tmin, tmax, g, so);
    CRANE_TSTAMP(a.trace, wg, 2);
    // ---- B: slots (wave prefix sums, the waves' totals exchanged once: one barrier)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t w0 = g[0].word(), w1 = g[1].word(), w2 = (g[0].cnt | g[1].cnt) ? 1u : 0u;
    uint32_t e0 = wave_scan_add(w0), e1 = wave_scan_add(w1), e2 = wave_scan_add(w2);
    // the flat maxima per wave go out with the totals (step_publish's exchange: one barrier for both)
    const int32_t fm0 = wave_max(so.flat0), fm1 = wave_max(so.flat1);
    if (lane == 0) {
        ssh.fm[0][wv] = fm0;
        ssh.fm[1][wv] = fm1;
    }
    if (lane == 63) {
        xch[0][wv] = e0;
        xch[1][wv] = e1;
        xch[2][wv] = e2;
    }
    e0 -= w0;
    e1 -= w1;
    e2 -= w2;
    __syncthreads();
    uint32_t base[3], tot[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint4 x = *reinterpret_cast<const uint4*>(xch[k]);
        base[k] = (wv > 0 ? x.x : 0u) + (wv > 1 ? x.y : 0u) + (wv > 2 ? x.z : 0u);
        tot[k] = x.x + x.y + x.z + x.w;
    }
    step_slots(g, base[0] + e0, base[1] + e1, so);
    const int32_t rs = (int32_t)(base[2] + e2);  // rank among the block's stepped nodes
    const int32_t nst = (int32_t)tot[2];
    if (threadIdx.x == 0) {
        ssh.lc[0][0] = (int32_t)(tot[0] & 0xFFFF);
        ssh.lc[0][1] = (int32_t)(tot[0] >> 16);
        ssh.lc[1][0] = (int32_t)(tot[1] & 0xFFFF);
        ssh.lc[1][1] = (int32_t)(tot[1] >> 16);
    }
    // step_publish's stores from the exchanged values (ssh.lc is read after the next barrier)
    step_publish_store<BS>(ssh, step.st, blk, [&](int L) {
        return (int32_t)((L & 1) ? tot[L >> 1] >> 16 : tot[L >> 1] & 0xFFFF);
    });
    // one-step records staged in LDS, or (more of a kind than it holds) in st.stage
    const bool g1 = (int32_t)max(tot[0] & 0xFFFF, tot[1] & 0xFFFF) > min(kSCap, step.st.lds_cap);
    CRANE_TSTAMP(a.trace, wg, 3);
    const S1Out s1o{s1l, step.st.stage + blk * 2 * step.st.bs, g1, (int64_t)kSCap, step.st.s1pad};
    // ---- C: the stepped nodes' records in LDS, chunk by chunk, and their (node, kind) items.
    // The first kSRec stepped nodes write their part (e_fail, pen, e_hv, slots) into the LDS
    // records now; any further ones into their node's record slot in HBM (step.srec, the node
    // records the keys-only step leaves stale anyway: the slots go in e_pred, which the emit does
    // not read), fetched chunk by chunk — no per-lane state lives across the chunks.
    const bool stepped = (g[0].cnt | g[1].cnt) != 0;
    auto put = [&](Rec* r) {  // (called with an LDS and a global pointer: no flat stores)
        r->e_fail = e_fail;
        r->pen = hr.pen;
        r->e_hv = hr.e_hv;
#pragma unroll
        for (int k = 0; k < PR; ++k) {
            r->e_prio[k] = ep[k];
            r->t[k] = tp[k];
        }
        int32_t* dw = reinterpret_cast<int32_t*>(r->e_pred);
        dw[0] = so.slot0;
        dw[1] = so.mslot0;
        dw[2] = so.slot1;
        dw[3] = so.mslot1;
        dw[4] = (so.multi0 ? 1 : 0) | (so.multi1 ? 2 : 0);
        dw[5] = s0;  // score_at(tmin): the keys before a node's first step
    };
    if (stepped && !(K1S_SKIP & 4)) {
        rank_lane[rs] = (uint8_t)threadIdx.x;
        if (rs < kSRec) put(&lrec[rs]);
        else put(static_cast<Rec*>(step.srec) + n);
    }
    __syncthreads();
    // a grid of many rounds: the epilogue's single-wave phases run on wave 0 alone and the other
    // waves leave, so their slots take the next workgroups' streams — before the emit when its
    // tasks fit one wave, else before the tail; a grid of one or two rounds keeps all four waves
    // (its time is one workgroup's chain)
    const bool t1 = K1S_TAIL1 && (step.tail1 == 1 || (step.tail1 == 0 && nwg >= 4096));
    const bool emit1 = t1 && nst * (PR + 2) <= 64;  // (workgroup-uniform)
    if (emit1 && threadIdx.x >= 64) return;
    const int nthr = emit1 ? 64 : BS;
#if K1S_RTAIL
    // few one-step records, staged in LDS, no elementary pieces (workgroup-uniform): the tail runs
    // in registers (small_tail); its first tile bounds load now, behind the emit
    const int32_t n0 = (int32_t)(tot[0] & 0xFFFF), n1 = (int32_t)(tot[1] & 0xFFFF);
    const bool small = !g1 && max(n0, n1) <= kSmallTail && !step.st.prow && !(K1S_SKIP & 2);
    const bool srows = step.st.rows && !(K1S_SKIP & 16);
    int64_t tpre[2] = {0, 0};
    if (small && srows && threadIdx.x < (t1 ? 64 : 128)) {
        if (t1) small_tail_bounds<true>(step.st, tpre);
        else small_tail_bounds<false>(step.st, tpre);
    }
#endif
    for (int32_t c0 = 0; c0 < ((K1S_SKIP & 1) ? 0 : nst); c0 += kSRec) {  // (workgroup-uniform)
        const int32_t m = min(kSRec, nst - c0);
        if (c0 > 0) {  // this chunk's records from HBM (L2: written by this workgroup)
            constexpr int W = 3 + 2 * PR + 3;  // e_fail, e_hv, pen, e_prio, t, then the slot words
            for (int i = threadIdx.x; i < m * W; i += BS) {
                const int j = i / W, f = i - j * W;
                const int64_t* src = reinterpret_cast<const int64_t*>(static_cast<const Rec*>(step.srec) + first +
                                                                      rank_lane[c0 + j]);
                reinterpret_cast<int64_t*>(&lrec[j])[f] = src[f];
            }
            __syncthreads();
        }
        {
            constexpr int NB = PR + 2;
            for (int tk = threadIdx.x; tk < m * NB; tk += nthr) {  // (node, candidate): both kinds
                const int j = tk / NB;
                int q = tk - j * NB;
                // (q = threadIdx.x % NB in every trip: without this the compiler hoists emit_task's
                // per-q lane masks out of the loop and spills them, ~30 SGPRs for the whole kernel)
                asm volatile("" : "+v"(q));
                emit_task<PD, PR>(lrec[j], first + rank_lane[c0 + j], q,
                                  reinterpret_cast<const int32_t*>(lrec[j].e_pred), tmin, tmax, step.wsum, step.noprio,
                                  step.st, blk, s1o, step.winv);
            }
        }
        __syncthreads();  // (the chunk's records are reused by the next chunk)
    }
    CRANE_TSTAMP(a.trace, wg, 5);
    // ---- D: the fused pass's tail
    if (K1S_SKIP & 2) return;
#if K1S_RTAIL
    if (small) {  // (workgroup-uniform) wave T takes kind T, or wave 0 both; the other waves leave
        if (threadIdx.x >= (t1 ? 64 : 128)) return;
        if (t1) small_tail<true>(s1l, n0, n1, ssh, step, blk, tpre, srows, a.trace, wg);
        else small_tail<false>(s1l, n0, n1, ssh, step, blk, tpre, srows, a.trace, wg);
        return;
    }
#endif
    if (t1) {
        if (threadIdx.x >= 64) return;
        if (threadIdx.x < 2) {  // the block's flat maxima into wave 0's slot (tile rows read it)
            const int T = threadIdx.x;
            ssh.fm[T][0] = block_flat_max<BS>(ssh, T);
        }
        tail<64>(g1, lrec, s1l, srt, ssh, step, blk, a.trace, wg);
        return;
    }
    tail<BS>(g1, lrec, s1l, srt, ssh, step, blk, a.trace, wg);
}

}  // namespace crane
