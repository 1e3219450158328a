// tm_retain_page.h -- tm_retained_match_page's batch descriptor and launchers
// (tm_retain_page.hip, tm_retain_page_host.cpp; tests/retain_cpu has the
// launchers in plain C++).  A page is the first `limit` hits of a filter in scan
// order: the base range of its literal prefix by ascending row, then the tail by
// ascending row, both clipped by the cursor and by the scan window.
//
// Three passes and no atomic: k_retp_count stores every tile's hit count,
// k_retp_cut turns one filter's counts into exclusive counts up to the tile in
// whose chunk `limit` is reached, k_retp_emit tests the rows of the tiles before
// the cut again and ranks the hits in row order.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "tm_retain.h"

namespace tmx {

constexpr uint32_t RTP_CHUNK = 256;   // tiles k_retp_cut takes per step: one per thread

// one filter of a page batch that has rows to scan.  A cursor starts a segment anywhere, so both are explicit
struct RetPQ {
    uint32_t nlev;        // levels without a final '#'
    uint32_t flags;       // RQ_*
    uint32_t skip;        // leading literal levels every row of [lo, hi) is known to equal
    uint32_t ids_off;     // its nlev level ids (RT_PLUS: '+') start here in the batch's id array
    uint64_t lo, hi;      // the base rows to scan: inside the range of its literal prefix
    uint64_t tail_lo, tail_hi;   // the tail rows to scan: inside [base, base + tail)
    uint32_t base_tiles;  // ceil((hi - lo) / RT_TILE)
    uint32_t tail_tiles;  // ceil((tail_hi - tail_lo) / RT_TILE); they follow the base tiles
};

// d_tile_cnt[t] = the hits in tile t of the batch, for t in [tile_base, tile_base + tiles), tiles <=
// RT_MAX_LAUNCH_TILES: every tile's word is stored (0 included), so the array needs no clearing
hipError_t launch_retp_count(const RetView &v, const RetPQ *d_q, uint32_t nq, const uint32_t *d_ids, const uint32_t *d_tile_ps,
                             uint32_t tile_base, uint32_t tiles, uint64_t now, uint32_t *d_tile_cnt, hipStream_t s);
// per filter f: d_tile_excl[t] = the hits of f's tiles before t, for f's tiles up to the end of the chunk of
// RTP_CHUNK tiles in which the sum reaches `limit`, and `limit` ("nothing to emit") for the tiles after;
// d_taken[f] = min(sum, limit); d_next_row[f] = 0
hipError_t launch_retp_cut(const uint32_t *d_tile_ps, uint32_t nq, const uint32_t *d_tile_cnt, uint32_t limit,
                           uint32_t *d_tile_excl, uint32_t *d_taken, uint64_t *d_next_row, hipStream_t s);
// the tiles [tile_base, tile_base + tiles) again: hit k of filter f in scan order, k < limit, goes to
// d_out[d_offs[f] + k] (nothing at or past out_cap); the row after hit limit - 1 to d_next_row[f]
hipError_t launch_retp_emit(const RetView &v, const RetPQ *d_q, uint32_t nq, const uint32_t *d_ids, const uint32_t *d_tile_ps,
                            uint32_t tile_base, uint32_t tiles, uint64_t now, uint32_t limit, const uint32_t *d_tile_cnt,
                            const uint32_t *d_tile_excl, const uint64_t *d_offs, uint32_t *d_out, uint64_t out_cap,
                            uint64_t *d_next_row, hipStream_t s);

}  // namespace tmx
