// topk.hip — the k best feasible nodes of every pod of a batch (crane_dyn_topk): per pod the
// k largest packed keys (score << 32 | 0xFFFFFFFF - global node, the keys of
// crane_dyn_eval_keys_async), best first, -1 where the pod has fewer feasible nodes — the
// runner-up candidates of a pod without the P x N matrices (matrix.hip) they could be ranked from.
//
// Evaluation is the per-pair kernels' lane cache (pair_eval.hpp) with the two keys of a node (per pod
// kind) as its value, from the same literal restatement (step_node.hpp: score_at and the Filter of
// key_of, now < e_fail; no score or filter arithmetic is restated here): a lane owns one node of a
// 256-node block and evaluates it at the minimum time of a 64-pod sub-chunk.
//
// Phase 1 (k_topk): a workgroup takes a chunk of CH pods and a slice of whole node blocks.  Every
// (wave, pod) has a sorted list of KC keys in LDS (KC = 4, 8, 16: the smallest >= k), stored
// [wave][entry][pod] so that 64 pods' entries are 64 consecutive words; entry KC - 1 is the pod's
// threshold.  Per block and 64-pod sub-chunk the wave changes sides: the lanes that evaluated 64
// nodes become the sub-chunk's 64 pods (time, kind, threshold in registers), and nodes are
// offered to all pods at once:
//   - the nodes without a step inside the sub-chunk have one key per pod kind for all its pods:
//     they are offered best first (a wave maximum, then the next), per kind, until no pod of the
//     kind takes one — one wave maximum and one ballot per kind once the lists have filled;
//   - a node with one step is broadcast (v_readlane of its step time and its keys before / after)
//     and every pod selects by its own time; one with several steps is read again through the
//     scalar path (a uniform record) and evaluated at the 64 pod times.
// A pod takes an offered key above its threshold by an insertion into its list in registers
// (3 selects per entry, all pods of the wave in parallel); the lists are read from LDS at the
// first offer a pod takes and written back once per sub-chunk.  At the end a thread per pod merges
// the four waves' lists, widens the keys and writes k of them with plain stores: to the output
// with one slice, else to partial[pod][slice][k].
// Phase 2 (k_topk_merge, S > 1): a wave per pod takes k times the largest of the S * k partial
// keys below the one before.  No atomics anywhere: the result does not depend on the order.
//
// List keys are 32-bit, pack_key(score, node index within the slice): a slice holds at most 2^24
// nodes.  The automatic slice count keeps to that for any shard; a forced count (engine option
// topk_slices) that would leave larger slices is rejected (CRANE_E_INVALID).
//
// LDS: 32 KiB of lists (CH = 2048 / KC pods: 512, 256, 128) and the chunk's times, flags and
// sub-chunk ranges: 33.5 - 38.1 KiB, under the default limit with no function attribute.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "dyn_types.hpp"
#include "kernels.hpp"
#include "step_node.hpp"
#include "pair_eval.hpp"

namespace crane {

constexpr int kTkT = 256;            // threads per workgroup = nodes per block
constexpr int kTkListWords = 8192;   // list entries per workgroup (4 waves x CH pods x KC)
constexpr int64_t kTkSliceMax = (int64_t)1 << 24;  // nodes per slice (pack_key's index bits)
// workgroups per compute unit the automatic slice count aims at, with at least kTkMinBlk node
// blocks per slice: every slice fills the lists of its chunk's pods before its thresholds skip
// anything, and writes k partial keys per pod for the second phase to read
constexpr int kTkWgPerCu = 2;
constexpr int kTkMinBlk = 8;

// the cached value: a node's list keys for the pods the Filter applies to (kn) and DaemonSet pods (kd)
struct TkKeys {
    int32_t kn = -1, kd = -1;  // (-1: not a candidate — a lane without a node)
};
template <int PD, int PR>
struct TkEval {
    double wsum;
    int32_t noprio;
    int64_t loc;  // the node's index within the slice
    __device__ __forceinline__ TkKeys operator()(int64_t t, const NodeRec<PD, PR>& r) const {
        const int32_t sc = score_at<PD, PR>(t, r, wsum, noprio);
        return {key_of<PD, PR>(0, t, sc, r, loc), key_of<PD, PR>(1, t, sc, r, loc)};
    }
};

template <int PD, int PR, int KC>
__global__ __launch_bounds__(kTkT) void k_topk(TopkArgs a) {
    constexpr int CH = kTkListWords / (4 * KC);  // pods per workgroup
    constexpr int NSC = CH / 64;                 // 64-pod sub-chunks
    static_assert(CH % 64 == 0 && KC <= 16, "whole sub-chunks; a list within one DPP row");
    static_assert(kTkListWords * 4 + CH * 12 + NSC * 16 <= 64 * 1024, "LDS within the default limit");
    __shared__ int32_t list[4 * CH * KC];  // [wave][KC][pod] descending over KC, -1 = empty; row KC - 1: the thresholds
    __shared__ int64_t tnow[CH];
    __shared__ int32_t tfl[CH];
    __shared__ int64_t scmin[NSC], scmax[NSC];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int64_t c = blockIdx.x / (uint32_t)a.S, s = blockIdx.x % (uint32_t)a.S;
    const int64_t p0 = c * CH;
    const int nlive = (int)min((int64_t)CH, a.P - p0);
    const int nsc = (nlive + 63) >> 6;

    for (int i = tid; i < 4 * CH * KC; i += kTkT) list[i] = -1;
    for (int i = tid; i < CH; i += kTkT) {
        tnow[i] = i < nlive ? a.now[p0 + i] : 0;
        tfl[i] = i < nlive && a.flags ? (int32_t)(a.flags[p0 + i] & 1u) : 0;
    }
    for (int q = w; q < nsc; q += 4) {  // the sub-chunks' time ranges
        const int i = q * 64 + lane;
        const int64_t tn = i < nlive ? a.now[p0 + i] : 0;
        int64_t mn, mx;
        subchunk_range(i < nlive, tn, mn, mx);
        if (lane == 0) {
            scmin[q] = mn;
            scmax[q] = mx;
        }
    }
    __syncthreads();

    // ---- the node slice: blocks [b0, b1) of the shard's nblk, keys by the index within it
    const int64_t nblk = (a.N + kTkT - 1) / kTkT;
    const int64_t b0 = s * nblk / a.S, b1 = (s + 1) * nblk / a.S;
    const NodeRec<PD, PR>* __restrict__ rec = static_cast<const NodeRec<PD, PR>*>(a.rec);
    int32_t* const wl = list + w * CH * KC;
    const int64_t loc0 = w * 64;  // the wave's first node within a block

    for (int64_t nb = b0; nb < b1; ++nb) {
        const int64_t n = nb * kTkT + tid;
        const bool valid = n < a.N;
        const int64_t locb = (nb - b0) * kTkT + loc0;  // the wave's first node within the slice
        const int64_t loc = locb + lane;
        // lane = node: its keys per pod kind, cached over the sub-chunks
        PairCache<TkKeys> c;
        for (int q = 0; q < nsc; ++q) {
            const int nv = min(64, nlive - q * 64);
            const int64_t cmin = scmin[q], cmax = scmax[q];
            if (valid && !c.covers(cmin, cmax)) {
                const NodeRec<PD, PR> r = rec[n];
                c.refresh(r, cmin, cmax, TkEval<PD, PR>{a.wsum, a.noprio, loc});
            }
            const bool stepped = c.bp <= cmax;  // (reused keys of an earlier sub-chunk's stepped node: bp = hi > cmax)
            uint64_t smask = __ballot(stepped);

            // lane = pod from here: its time, kind, threshold and (once an offer is taken) its list
            int32_t* const L = wl + q * 64 + lane;  // entry i at L[i * CH]
            const int64_t tn = tnow[q * 64 + lane];
            const bool ds = tfl[q * 64 + lane] != 0;
            const bool live = lane < nv;
            int32_t th = L[(KC - 1) * CH];
            int32_t e[KC];
            bool have = false;  // (uniform)
            // one node's key per pod (-1: not for this pod) into the lists it beats the threshold of;
            // false when no pod took it.  Every lane calls this.
            auto offer = [&](int32_t cand) {
                const bool take = live && cand > th;
                if (__ballot(take) == 0) return false;
                if (!have) {
#pragma unroll
                    for (int i = 0; i < KC; ++i) e[i] = L[i * CH];
                    have = true;
                }
                if (take) {
#pragma unroll
                    for (int i = KC - 1; i >= 1; --i) e[i] = e[i] >= cand ? e[i] : (e[i - 1] >= cand ? cand : e[i - 1]);
                    e[0] = max(e[0], cand);
                    th = e[KC - 1];
                }
                return true;
            };

            // the nodes without a step: their keys hold for every pod of a kind, so they are offered
            // best first (wave maximum, then the next) until no pod of the kind takes one
            int32_t rn = stepped ? -1 : c.v0.kn, rd = stepped ? -1 : c.v0.kd;
            if (__ballot(live && !ds) != 0) {
                for (;;) {
                    const int32_t c = wave_max(rn);
                    if (c < 0 || !offer(ds ? -1 : c)) break;
                    if (rn == c) rn = -1;  // (the keys of two nodes differ)
                }
            }
            if (__ballot(live && ds) != 0) {
                for (;;) {
                    const int32_t c = wave_max(rd);
                    if (c < 0 || !offer(ds ? c : -1)) break;
                    if (rd == c) rd = -1;
                }
            }
            // the stepped nodes one by one: 64 pods at a time against the node's keys before / after
            // its step, or (several steps) its record through the scalar path and the pod's own time
            while (smask) {
                const int j = __builtin_ctzll(smask);
                smask &= smask - 1;
                PairCache<TkKeys> b;  // node j's, uniform
                b.multi = __builtin_amdgcn_readlane((int)c.multi, j) != 0;
                b.bp = readlane64(c.bp, j);
                b.v0 = {__builtin_amdgcn_readlane(c.v0.kn, j), __builtin_amdgcn_readlane(c.v0.kd, j)};
                b.v1 = {__builtin_amdgcn_readlane(c.v1.kn, j), __builtin_amdgcn_readlane(c.v1.kd, j)};
                const TkKeys x = b.at(tn, rec + nb * kTkT + w * 64 + j, TkEval<PD, PR>{a.wsum, a.noprio, locb + j});
                offer(ds ? x.kd : x.kn);
            }
            if (have) {
#pragma unroll
                for (int i = 0; i < KC; ++i) L[i * CH] = e[i];
            }
        }
    }
    __syncthreads();

    // ---- per pod: the four waves' lists merged, as 64-bit keys of global node indices
    const int k = a.k;
    const int64_t g0 = a.node_offset + b0 * kTkT;
    for (int i = tid; i < nlive; i += kTkT) {
        long long* __restrict__ o = a.S == 1 ? a.out + (p0 + i) * k : a.partial + ((p0 + i) * a.S + s) * k;
        int h0 = 0, h1 = 0, h2 = 0, h3 = 0;  // heads of the waves' lists
        const int32_t* const l0 = list + 0 * CH * KC + i;  // entry h at [h * CH]
        const int32_t* const l1 = list + 1 * CH * KC + i;
        const int32_t* const l2 = list + 2 * CH * KC + i;
        const int32_t* const l3 = list + 3 * CH * KC + i;
        for (int x = 0; x < k; ++x) {
            const int32_t v0 = h0 < KC ? l0[h0 * CH] : -1, v1 = h1 < KC ? l1[h1 * CH] : -1;
            const int32_t v2 = h2 < KC ? l2[h2 * CH] : -1, v3 = h3 < KC ? l3[h3 * CH] : -1;
            const int32_t m = max(max(v0, v1), max(v2, v3));
            long long key = -1;
            if (m >= 0) {
                if (v0 == m) ++h0;
                else if (v1 == m) ++h1;
                else if (v2 == m) ++h2;
                else ++h3;
                key = wide_key_of(m, g0);
            }
            o[x] = key;
        }
    }
}

// Phase 2: row p = the k largest of partial[p][0 .. S * k), descending, -1 past the last.  The
// slices' keys are distinct (distinct nodes), so "the largest below the previous" walks them in order.
__global__ __launch_bounds__(kTkT) void k_topk_merge(const long long* __restrict__ partial, int64_t P, int32_t S,
                                                     int32_t k, long long* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * (kTkT / 64) + (threadIdx.x >> 6);
    if (p >= P) return;  // (a whole wave)
    const int64_t tot = (int64_t)S * k;
    const long long* __restrict__ row = partial + p * tot;
    long long prev = INT64_MAX;
    for (int x = 0; x < k; ++x) {
        long long m = -1;
        if (prev >= 0) {
            for (int64_t e = lane; e < tot; e += 64) {
                const long long v = row[e];
                if (v < prev) m = max(m, v);
            }
            m = wave_max64(m);
        }
        if (lane == 0) out[p * k + x] = m;
        prev = m;
    }
}

static int topk_chunk(int k) { return kTkListWords / (4 * (k <= 4 ? 4 : k <= 8 ? 8 : 16)); }

int64_t topk_slices(int64_t P, int64_t N, int k, int slices, int n_cu) {
    if (P <= 0 || N <= 0) return 1;
    const int64_t chunks = (P + topk_chunk(k) - 1) / topk_chunk(k), nblk = (N + kTkT - 1) / kTkT;
    const int64_t smin = (nblk * kTkT + kTkSliceMax - 1) / kTkSliceMax;  // slices of at most 2^24 nodes
    int64_t S = slices;
    if (S <= 0) {
        S = std::min<int64_t>(std::max<int64_t>(1, (int64_t)kTkWgPerCu * std::max(n_cu, 1) / chunks),
                              nblk / kTkMinBlk);
        S = std::max(S, smin);
    }
    S = std::max<int64_t>(1, std::min(S, nblk));
    if (S < smin || chunks * S > 0x7FFFFFFFLL || S * k > 0x7FFFFFFFLL) return -1;
    return S;
}

hipError_t launch_topk(int shape, const TopkArgs& a, hipStream_t st) {
    if (a.P <= 0) return hipSuccess;
    if (a.k < 1 || a.k > 16 || a.S < 1 || (a.S > 1 && !a.partial)) return hipErrorInvalidValue;
    if (a.N <= 0) return hipMemsetAsync(a.out, 0xFF, sizeof(long long) * (size_t)a.P * (size_t)a.k, st);
    const dim3 g((unsigned)((a.P + topk_chunk(a.k) - 1) / topk_chunk(a.k) * a.S)), b(kTkT);
    const hipError_t e = with_shape(shape, [&](auto pd, auto pr) {
        if (a.k <= 4) return klaunch("k_topk", k_topk<pd(), pr(), 4>, g, b, 0, st, a);
        if (a.k <= 8) return klaunch("k_topk", k_topk<pd(), pr(), 8>, g, b, 0, st, a);
        return klaunch("k_topk", k_topk<pd(), pr(), 16>, g, b, 0, st, a);
    });
    if (e != hipSuccess || a.S == 1) return e;
    return klaunch("k_topk_merge", k_topk_merge, dim3((unsigned)((a.P + kTkT / 64 - 1) / (kTkT / 64))), dim3(kTkT), 0, st,
                   (const long long*)a.partial, a.P, a.S, a.k, a.out);
}

}  // namespace crane
