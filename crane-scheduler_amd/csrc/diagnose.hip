// diagnose.hip — the Filter's diagnosis for a pod batch (plugins.go:39-69): per pod, how
// many of the shard's nodes fail first at each predicate and how many pass — the counts
// kube-scheduler's FitError prints ("0/N nodes are available: k ...") — without the
// P x N first-fail matrix (matrix.hip) they could be histogrammed from.
//
// Predicate k fails iff now < e_pred[k] (dyn_types.hpp), so with the prefix maxima
// m_k = max_{j <= k} e_pred[j] (m_{-1} = INT64_MIN) a node's first failing predicate at `now`
// is k iff m_{k-1} <= now < m_k.  Per pod only C_k(now) = #{nodes : m_k <= now} is needed:
// the count of k is C_{k-1} - C_k (C_{-1} = n) and the feasible count is C_{npd-1}.  C_k is
// the rank of `now` among the nodes' m_k.
//
// A workgroup takes a pod tile and a node slice (whole 256-node blocks).  It sorts the tile's
// times in LDS (all pods in one order: the DaemonSet bypass is applied at the output), then
// its lanes stream the slice, one node per lane per round: the node's predicate rows
// (ts, val) give e_pred[k] with rec_metrics' own expressions (node_rec.hpp pred_expiry), and
// per k the node adds 1 to a difference row diff[k][lower_bound(times, m_k)] — position 0
// for a node that counts for every pod of the tile (one add per wave), nothing for one that
// counts for none.  A prefix sum of each row over the sorted positions is C_k per pod; each
// pod writes its n_pred + 1 columns through its original position: plain stores with one
// slice per tile, int32 atomic adds into a zeroed output with several (integer sums: the
// result does not depend on the order).
//
// LDS: the sorted times and positions (12 B per pod) and npd rows of TILE + 1 int32.  Up to
// 8 device predicates take 1024-pod tiles (44.4 KiB); the 16-predicate instance takes
// 512-pod tiles (38.6 KiB) — one pass over the nodes, no function attribute.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "dyn_types.hpp"
#include "kernels.hpp"
#include "node_rec.hpp"

namespace crane {

constexpr int kDgT = 256;     // threads per workgroup = nodes per block
// workgroups per compute unit the automatic slice count aims at: a slice repeats its tile's sort,
// prefix sums and output, so more slices than fill the device once cost more than their shorter
// node streams save (config 3: 24-32 slices 0.046 ms, 96 0.091, 8 0.076; profiles/ab/filter_counts.txt)
constexpr int kDgWgPerCu = 1;
constexpr int kDgMinBlk = 4;  // ... with at least this many node blocks per slice

template <int PD, int TILE>
__global__ __launch_bounds__(kDgT) void k_filter_counts(DiagArgs a) {
    static_assert(TILE % kDgT == 0 && (TILE & (TILE - 1)) == 0, "a tile is a power of two of whole rounds");
    constexpr int kU = TILE / kDgT;  // pods per lane
    constexpr int kLd = TILE + 1;    // difference row stride
    constexpr int kW = kDgT / 64;
    constexpr uint64_t kSign = 1ull << 63;
    static_assert(TILE * 12 + PD * kLd * 4 + PD * kW * 4 <= 64 * 1024, "LDS within the default limit");
    __shared__ uint64_t ku[TILE];      // now ^ sign, ascending: unsigned order = signed order
    __shared__ uint32_t kv[TILE];      // the pod's position in the tile
    __shared__ int32_t diff[PD * kLd]; // per device predicate: adds by sorted position, then C_k
    __shared__ int32_t wsum[PD][kW];
    const DevPolicy& pol = a.pol;
    const int npd = min(pol.npd, PD);
    const int64_t t = blockIdx.x / (uint32_t)a.S, s = blockIdx.x % (uint32_t)a.S;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int64_t p0 = t * TILE;
    const int nlive = (int)min((int64_t)TILE, a.P - p0);

    // ---- the tile's times, sorted (slots past the batch sort last and are never written out)
    bool inorder = true;
#pragma unroll
    for (int u = 0; u < kU; ++u) {
        const int i = u * kDgT + tid;
        const int64_t tn = i < nlive ? a.now[p0 + i] : INT64_MAX;
        if (i + 1 < nlive) inorder &= tn <= a.now[p0 + i + 1];
        ku[i] = i < nlive ? (uint64_t)tn ^ kSign : ~0ull;
        kv[i] = (uint32_t)i;
    }
    for (int j = tid; j < npd * kLd; j += kDgT) diff[j] = 0;
    if (!__syncthreads_and(inorder)) {
        // bitonic sort of the (time, position) pairs; equal times keep any order (the counts
        // of equal times are equal)
        for (int k = 2; k <= TILE; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int q = tid; q < TILE / 2; q += kDgT) {
                    const int i = ((q & ~(j - 1)) << 1) | (q & (j - 1)), l = i | j;
                    const uint64_t ka = ku[i], kb = ku[l];
                    if (ka != kb && (ka > kb) == ((i & k) == 0)) {
                        const uint32_t va = kv[i], vb = kv[l];
                        ku[i] = kb;
                        ku[l] = ka;
                        kv[i] = vb;
                        kv[l] = va;
                    }
                }
                __syncthreads();
            }
        }
    }
    const uint64_t kmin = ku[0], kmax = ku[nlive - 1];

    // ---- the node slice: blocks [b0, b1) of the shard's nblk
    const int64_t nblk = (a.N + kDgT - 1) / kDgT;
    const int64_t b0 = s * nblk / a.S, b1 = (s + 1) * nblk / a.S;
    const int64_t n0 = b0 * kDgT, n1 = min(a.N, b1 * kDgT);
    if (npd > 0) {
        for (int64_t nb = n0; nb < n1; nb += kDgT) {
            const bool valid = nb + tid < n1;
            const int64_t n = min(nb + tid, n1 - 1);  // (clamped: the loads are unconditional)
            int64_t pt[PD];
            double pv[PD];
#pragma unroll
            for (int k = 0; k < PD; ++k) {
                const int64_t row = k < npd ? pol.pred_slot[k] : 0;
                pt[k] = k < npd ? a.ts[row * a.N + n] : kTsInvalid;
                pv[k] = k < npd ? a.val[row * a.N + n] : 0.0;
            }
            // m = m_k so far; pos = lower_bound(times, m): the first sorted pod with now >= m
            // (0: every pod of the tile, -1: none).  Searched again only where m_k > m_{k-1}.
            int64_t m = kTsInvalid;
            int32_t pos = 0;
#pragma unroll
            for (int k = 0; k < PD; ++k) {
                if (k >= npd) continue;  // (uniform)
                const int64_t e = pred_expiry(pol, k, pt[k], pv[k]);
                if (e > m) {
                    m = e;
                    const uint64_t mk = (uint64_t)m ^ kSign;
                    if (mk <= kmin) {
                        pos = 0;
                    } else if (mk > kmax) {
                        pos = -1;
                    } else {
                        int lo = 0, hi = nlive - 1;  // ku[lo] < mk <= ku[hi]
                        while (hi - lo > 1) {
                            const int mid = (lo + hi) >> 1;
                            if (ku[mid] < mk) lo = mid;
                            else hi = mid;
                        }
                        pos = hi;
                    }
                }
                const uint64_t all = __ballot(valid && pos == 0);
                if (lane == 0 && all) atomicAdd(&diff[k * kLd], (int32_t)__popcll(all));
                if (valid && pos > 0) atomicAdd(&diff[k * kLd + pos], 1);
            }
        }
    }
    __syncthreads();

    // ---- C_k per sorted position: a block prefix sum of every row, in place
    {
        int32_t v[PD][kU], run[PD];
#pragma unroll
        for (int k = 0; k < PD; ++k) {
            if (k >= npd) continue;
            int32_t acc = 0;
#pragma unroll
            for (int u = 0; u < kU; ++u) {
                acc += diff[k * kLd + tid * kU + u];
                v[k][u] = acc;
            }
            int32_t sc = acc;  // inclusive scan of the lanes' sums over the wave
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int32_t x = __shfl_up(sc, o);
                if (lane >= o) sc += x;
            }
            if (lane == 63) wsum[k][w] = sc;
            run[k] = sc - acc;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < PD; ++k) {
            if (k >= npd) continue;
            int32_t off = run[k];
            for (int x = 0; x < w; ++x) off += wsum[k][x];
#pragma unroll
            for (int u = 0; u < kU; ++u) diff[k * kLd + tid * kU + u] = v[k][u] + off;
        }
        __syncthreads();
    }

    // ---- each pod's row through its original position
    const int32_t nsl = (int32_t)(n1 - n0);
    const int32_t np = a.n_pred;
    for (int i = tid; i < TILE; i += kDgT) {
        // (by position, not by rank: a pod at INT64_MAX ties with the slots past the batch)
        if (kv[i] >= (uint32_t)nlive) continue;
        const int64_t p = p0 + kv[i];
        const bool ds = a.flags && (a.flags[p] & 1u);  // Filter bypass (plugins.go:41-43)
        int32_t* __restrict__ row = a.counts + p * (np + 1);
        int32_t prev = nsl;
        int k = 0;
        for (int j = 0; j <= np; ++j) {
            int32_t x = 0;
            if (j == np) {
                x = ds ? nsl : prev;
            } else if (k < npd && a.pred_orig[k] == j) {
                const int32_t c = diff[k * kLd + i];
                x = ds ? 0 : prev - c;
                prev = c;
                ++k;
            }
            if (a.S == 1) row[j] = x;
            else if (x != 0) atomicAdd(&row[j], x);
        }
    }
}

// Pods per tile of the instance that takes npd device predicates
static int diag_tile(int npd) { return npd > 8 ? 512 : 1024; }

hipError_t launch_filter_counts(const DiagArgs& a0, int slices, int n_cu, hipStream_t st) {
    if (a0.P <= 0) return hipSuccess;
    const size_t bytes = sizeof(int32_t) * (size_t)a0.P * (size_t)(a0.n_pred + 1);
    if (a0.N <= 0) return hipMemsetAsync(a0.counts, 0, bytes, st);
    if (a0.N > 0x7FFFFFFFLL || a0.pol.npd > kMaxPred) return hipErrorInvalidValue;
    DiagArgs a = a0;
    const int npd = a.pol.npd, tile = diag_tile(npd);
    const int64_t tiles = (a.P + tile - 1) / tile, nblk = (a.N + kDgT - 1) / kDgT;
    int64_t S = slices;
    if (S <= 0) {
        // a few workgroups per compute unit, each slice long enough to carry the tile's sort and
        // output; from 8 on a multiple of 8, so that a slice's tiles run on one XCD (its L2)
        S = std::min<int64_t>(std::max<int64_t>(1, (int64_t)kDgWgPerCu * std::max(n_cu, 1) / tiles), nblk / kDgMinBlk);
        if (S >= 8) S &= ~(int64_t)7;
    }
    S = std::max<int64_t>(1, std::min(S, nblk));
    if (npd == 0) S = 1;  // no node is read: every row is {0, ..., N}
    if (tiles * S > 0x7FFFFFFFLL) return hipErrorInvalidValue;
    a.S = (int32_t)S;
    if (S > 1)
        if (hipError_t e = hipMemsetAsync(a.counts, 0, bytes, st)) return e;
    const dim3 g((unsigned)(tiles * S)), b(kDgT);
    if (npd <= 4) return klaunch("k_filter_counts", k_filter_counts<4, 1024>, g, b, 0, st, a);
    if (npd <= 8) return klaunch("k_filter_counts", k_filter_counts<8, 1024>, g, b, 0, st, a);
    return klaunch("k_filter_counts", k_filter_counts<16, 512>, g, b, 0, st, a);
}

}  // namespace crane
