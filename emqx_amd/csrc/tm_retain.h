// tm_retain.h -- the retained-message store's device layout and launchers
// (tm_retain.hip, tm_retain_host.cpp; tests/retain_cpu has the launchers in
// plain C++; the paged lookup's descriptor and launchers: tm_retain_page.h).  Independent of the topic index (tm_dev.h): one filter against
// many stored topic names, emqx_retainer_mnesia:match_messages/3.
//
// Rows are a column store.  A row's level words are u32 ids of an exact host
// dictionary; levels 0 .. RT_COLS-1 live in one column each (cols + l * stride),
// levels RT_COLS and deeper row-major in ovf at ovf_off[row].  Rows [0, base)
// are sorted by id sequence, rows [base, base + tail) are recent inserts in
// arrival order.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace tmx {

constexpr uint32_t RT_COLS = 8;     // levels kept in columns
constexpr uint32_t RT_TILE = 256;   // rows a block scans: one lane, one row
constexpr uint32_t RT_MAX_LEVELS = 65536;
// tiles one launch of k_ret_rows takes: HIP launches fewer than 2^32 threads (gridDim.x * blockDim.x), so a
// batch with more tiles is scanned by several launches, each told the first tile it owns.  (A build of the
// host side for the CPU device fake sets a small value to run that arithmetic on small batches.)
#ifndef RT_LAUNCH_TILES
#define RT_LAUNCH_TILES ((1u << 24) - 1)
#endif
constexpr uint32_t RT_MAX_LAUNCH_TILES = RT_LAUNCH_TILES;
static_assert((uint64_t)RT_MAX_LAUNCH_TILES * RT_TILE < (1ull << 32), "a launch has fewer than 2^32 threads");

// meta: the level count in the low 20 bits, flag bits above
constexpr uint32_t RT_NLEV_MASK = 0xFFFFFu;
constexpr uint32_t RT_LIVE = 1u << 28, RT_DOLLAR = 1u << 29, RT_HAS_EXPIRY = 1u << 30, RT_HAS_OVF = 1u << 31;

constexpr uint32_t RT_PLUS = 0xFFFFFFFFu;   // a filter level '+' (never a dictionary id)
// RetQ.flags
constexpr uint32_t RQ_HASH = 1u;            // the filter ends in '#' (not counted in nlev)
constexpr uint32_t RQ_WILD_FIRST = 2u;      // its first level is '+' or '#': no '$' topic (MQTT-4.7.2-1)

struct RetView {
    uint32_t *cols;       // RT_COLS columns of `stride` words
    uint64_t stride;      // rows allocated
    uint32_t *meta;
    uint32_t *value;
    uint64_t *expiry;     // read only for rows flagged RT_HAS_EXPIRY
    uint64_t *ovf_off;    // read only for rows flagged RT_HAS_OVF
    uint32_t *ovf;
    uint64_t ovf_cap;     // words allocated in ovf
    uint64_t base, tail;  // rows [0, base) sorted, [base, base + tail) in arrival order
};

// one filter of a match batch that has rows to scan
struct RetQ {
    uint32_t nlev;        // levels without a final '#'
    uint32_t flags;       // RQ_*
    uint32_t skip;        // leading literal levels every row of [lo, hi) is known to equal
    uint32_t ids_off;     // its nlev level ids (RT_PLUS: '+') start here in the batch's id array
    uint64_t lo, hi;      // the base range of its literal prefix
    uint32_t base_tiles;  // ceil((hi - lo) / RT_TILE); its tail tiles follow
    uint32_t pad;
};

// one write of k_ret_apply (one per row and launch)
struct RetOp {
    uint32_t row;
    uint32_t meta;
    uint32_t value;
    uint32_t nwords;      // > 0: an append, the row's level ids at words_off; 0: meta, value and expiry alone
    uint64_t expiry;
    uint64_t ovf_off;     // where levels RT_COLS.. go in ovf (nwords > RT_COLS)
    uint64_t words_off;
};

// k_ret_apply: the batch's writes, one launch
hipError_t launch_ret_apply(const RetView &v, const RetOp *d_ops, uint32_t n_ops, const uint32_t *d_words, uint64_t n_words,
                            hipStream_t s);
// count the hits in tiles [tile_base, tile_base + tiles) of the batch (tiles <= RT_MAX_LAUNCH_TILES), added to
// d_counts[nq], which the caller zeroed before the batch's first launch
hipError_t launch_ret_count(const RetView &v, const RetQ *d_q, uint32_t nq, const uint32_t *d_ids, const uint32_t *d_tile_ps,
                            uint32_t tile_base, uint32_t tiles, uint64_t now, uint32_t *d_counts, hipStream_t s);
// d_offs[nq + 1]: the exclusive sums of d_counts; d_cursor[nq] zeroed
hipError_t launch_ret_offsets(const uint32_t *d_counts, uint32_t nq, uint64_t *d_offs, uint32_t *d_cursor, hipStream_t s);
// the same scan again, launch by launch: hit k of filter q goes to d_out[d_offs[q] + k], k in an unspecified order
// (d_cursor carries on from launch to launch); nothing at or past out_cap
hipError_t launch_ret_emit(const RetView &v, const RetQ *d_q, uint32_t nq, const uint32_t *d_ids, const uint32_t *d_tile_ps,
                           uint32_t tile_base, uint32_t tiles, uint64_t now, const uint64_t *d_offs, uint32_t *d_cursor, uint32_t *d_out,
                           uint64_t out_cap, hipStream_t s);

}  // namespace tmx
