// topk_merge.cpp — the combine of node shards' top-k rows (crane_topk_merge): plain host code.
//
// Every input row is descending with its -1 pads last, so the k largest of the rows' union are a
// k-step merge over one head per list.  Keys of disjoint shards differ (global node indices); a
// key that two lists share anyway is kept once per list, as a sort of the concatenated rows would.
#include <stdint.h>

#include <vector>

#include "../../include/crane_dyn.h"

extern "C" int crane_topk_merge(int32_t n_lists, int64_t n_pods, int32_t k, const int64_t* const* lists,
                                int64_t* out) {
    if (n_lists < 1 || n_pods < 0 || k < 1 || k > CRANE_TOPK_MAX || !lists) return CRANE_E_INVALID;
    if (n_pods == 0) return CRANE_OK;
    if (!out) return CRANE_E_INVALID;
    for (int32_t l = 0; l < n_lists; ++l)
        if (!lists[l]) return CRANE_E_INVALID;
    std::vector<int32_t> head((size_t)n_lists);
    for (int64_t p = 0; p < n_pods; ++p) {
        const int64_t row = p * k;
        for (int32_t l = 0; l < n_lists; ++l) head[(size_t)l] = 0;
        for (int32_t j = 0; j < k; ++j) {
            int64_t best = -1;
            int32_t from = -1;
            for (int32_t l = 0; l < n_lists; ++l) {
                const int32_t h = head[(size_t)l];
                if (h < k && lists[l][row + h] > best) {
                    best = lists[l][row + h];
                    from = l;
                }
            }
            if (from >= 0) ++head[(size_t)from];
            out[row + j] = best < 0 ? -1 : best;
        }
    }
    return CRANE_OK;
}
