// tm_retain_dev.h -- the retained store's row test, for the two translation
// units that scan rows (tm_retain.hip: whole lists; tm_retain_page.hip: pages in
// scan order).  Device code only: include after <hip/hip_runtime.h>.
#pragma once
#include "tm_retain.h"

namespace tmx {

// does row `row` match filter q (levels skip .. nlev-1 still to test)?  Q: a batch descriptor with nlev, flags
// and ids_off (RetQ, RetPQ)
template <class Q>
__device__ __forceinline__ bool ret_row_matches(const RetView &v, const Q &q, const uint32_t *__restrict__ ids,
                                                uint32_t skip, uint64_t row, uint64_t now) {
    const uint32_t meta = v.meta[row];
    const uint32_t nlev = meta & RT_NLEV_MASK;
    bool ok = (meta & RT_LIVE) != 0;
    ok = ok && !((q.flags & RQ_WILD_FIRST) && (meta & RT_DOLLAR));
    ok = ok && ((q.flags & RQ_HASH) ? nlev >= q.nlev : nlev == q.nlev);
    // the level loop is uniform over the block; a lane that is out loads nothing more
    for (uint32_t l = skip; l < q.nlev; ++l) {
        const uint32_t want = ids[q.ids_off + l];
        if (want == RT_PLUS) continue;
        if (ok) {
            // nlev >= q.nlev > l: the row has this level (in ovf when l >= RT_COLS, and then it is flagged)
            const uint32_t have = l < RT_COLS ? v.cols[(uint64_t)l * v.stride + row] : v.ovf[v.ovf_off[row] + (l - RT_COLS)];
            ok = have == want;
        }
    }
    if (ok && (meta & RT_HAS_EXPIRY)) ok = v.expiry[row] > now;   // (:464-466; now == 0 shows every row)
    return ok;
}

}  // namespace tmx
