// fake_retain_page_launch.cpp -- the three tmx::launch_retp_* symbols
// tm_retain_page_host.cpp links against, in plain C++ over the CPU device fake
// (tests/host_cpu/fake_hip.cpp); fake_retain_launch.cpp has launch_ret_offsets.
//
// The launchers restate k_retp_count, k_retp_cut and k_retp_emit tile by tile.
// Like the match launchers they do not trust what the host promises.  Scan
// order (base range by ascending row, then the tail by ascending row) is
// ascending row index, since the base lies below the tail.  So for every filter
// the emit launcher that holds its last tile tests EVERY row of the image, all
// levels from the first, and aborts unless the matching rows from the first row
// the segments cover (the cursor) to the last (the window's end, or the end of
// the tail), cut at `limit`, are exactly the values the launches left in the
// filter's list, in that order: a matching row in a gap between the segments, a
// base segment outside the prefix range or a wrong rank all fail here.  A
// batch's tiles come in launches of at most RT_MAX_LAUNCH_TILES; a gap or an
// overlap between them is refused.  Every word read or written is checked
// against the allocation that holds it (fake_hip_room).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../emqx_amd/csrc/tm_retain_page.h"

extern "C" size_t fake_hip_room(const void *p);

namespace {

using namespace tmx;

[[noreturn]] void die(const char *what) {
    fprintf(stderr, "fake_retain_page_launch: %s\n", what);
    abort();
}

template <class T>
T rd(const T *p) {
    if (fake_hip_room(p) < sizeof(T)) die("a read outside every device allocation");
    return *p;
}

template <class T>
void wr(T *p, T x) {
    if (fake_hip_room(p) < sizeof(T)) die("a write outside every device allocation");
    *p = x;
}

uint32_t level_id(const RetView &v, uint64_t row, uint32_t l) {
    if (l < RT_COLS) return rd(v.cols + (uint64_t)l * v.stride + row);
    if (!(rd(v.meta + row) & RT_HAS_OVF)) die("a level past the columns of a row without overflow");
    const uint64_t at = rd(v.ovf_off + row) + (l - RT_COLS);
    if (at >= v.ovf_cap) die("an overflow run past the array");
    return rd(v.ovf + at);
}

// emqx_topic:match/2 over ids plus the match path's expiry rule, levels `from` .. (from == 0: the restatement)
bool row_matches(const RetView &v, const RetPQ &q, const uint32_t *ids, uint64_t row, uint32_t from, uint64_t now) {
    const uint32_t meta = rd(v.meta + row), nlev = meta & RT_NLEV_MASK;
    if (!(meta & RT_LIVE)) return false;
    if ((q.flags & RQ_WILD_FIRST) && (meta & RT_DOLLAR)) return false;
    if ((q.flags & RQ_HASH) ? nlev < q.nlev : nlev != q.nlev) return false;
    for (uint32_t l = from; l < q.nlev; ++l) {
        const uint32_t want = rd(ids + q.ids_off + l);
        if (want != RT_PLUS && level_id(v, row, l) != want) return false;
    }
    if ((meta & RT_HAS_EXPIRY) && !(rd(v.expiry + row) > now)) return false;
    return true;
}

void check_segments(const RetView &v, const RetPQ &q, const uint32_t *tps, uint32_t f) {
    const uint64_t n = v.base + v.tail;
    if (n > v.stride) die("more rows than the columns hold");
    if (q.lo > q.hi || q.hi > v.base) die("a base segment outside the base");
    if (q.tail_lo > q.tail_hi || q.tail_lo < v.base || q.tail_hi > n) die("a tail segment outside the tail");
    if (q.base_tiles != (q.hi - q.lo + RT_TILE - 1) / RT_TILE) die("base_tiles is not its segment's tile count");
    if (q.tail_tiles != (q.tail_hi - q.tail_lo + RT_TILE - 1) / RT_TILE) die("tail_tiles is not its segment's tile count");
    if (q.base_tiles + q.tail_tiles == 0) die("a filter without rows was launched");
    if (rd(tps + f + 1) - rd(tps + f) != q.base_tiles + q.tail_tiles) die("the tile prefix sums disagree with the segments");
    if (q.skip > q.nlev) die("more prefix levels than levels");
}

uint64_t g_next_count = 0, g_next_emit = 0;

void check_launch(uint64_t &next, const uint32_t *tps, uint32_t nq, uint32_t tile_base, uint32_t tiles) {
    if ((uint64_t)tiles * RT_TILE >= (1ull << 32)) die("a launch of 2^32 threads or more");
    if (tiles > RT_MAX_LAUNCH_TILES || tiles == 0) die("a launch of no tiles, or of more than RT_MAX_LAUNCH_TILES");
    if (rd(tps) != 0) die("the tile prefix sums do not start at 0");
    const uint64_t total = rd(tps + nq);
    if (tile_base != 0 && tile_base != next) die("a batch's launches leave a gap or overlap");
    if ((uint64_t)tile_base + tiles > total) die("a launch past the batch's tiles");
    if ((uint64_t)tile_base + tiles < total && tiles != RT_MAX_LAUNCH_TILES) die("a short launch that is not the batch's last");
    next = (uint64_t)tile_base + tiles;
}

// the rows of tile t (counted from the filter's first) that the kernel's test finds, in row order
std::vector<uint64_t> tile_hits(const RetView &v, const RetPQ &q, const uint32_t *ids, uint64_t t, uint64_t now) {
    const bool base = t < q.base_tiles;
    const uint64_t row0 = base ? q.lo + t * RT_TILE : q.tail_lo + (t - q.base_tiles) * RT_TILE;
    const uint64_t end = base ? q.hi : q.tail_hi;
    std::vector<uint64_t> out;
    for (uint64_t r = row0; r < row0 + RT_TILE && r < end; ++r)
        if (row_matches(v, q, ids, r, base ? q.skip : 0, now)) out.push_back(r);
    return out;
}

// every row of the image from the segments' first row to their last, all levels tested
std::vector<uint64_t> audited(const RetView &v, const RetPQ &q, const uint32_t *ids, uint64_t now) {
    const uint64_t first = q.base_tiles ? q.lo : q.tail_lo, last = q.tail_tiles ? q.tail_hi : q.hi;
    std::vector<uint64_t> out;
    for (uint64_t r = 0; r < v.base + v.tail; ++r) {
        if (!row_matches(v, q, ids, r, 0, now)) continue;
        const bool in_seg = (r >= q.lo && r < q.hi) || (r >= q.tail_lo && r < q.tail_hi);
        if (r >= first && r < last) {
            if (!in_seg) die("a matching row between the cursor and the window's end lies outside the segments");
            out.push_back(r);
        }
    }
    return out;
}

}  // namespace

namespace tmx {

hipError_t launch_retp_count(const RetView &v, const RetPQ *d_q, uint32_t nq, const uint32_t *d_ids, const uint32_t *d_tile_ps,
                             uint32_t tile_base, uint32_t tiles, uint64_t now, uint32_t *d_tile_cnt, hipStream_t) {
    check_launch(g_next_count, d_tile_ps, nq, tile_base, tiles);
    for (uint32_t f = 0; f < nq; ++f) {
        const uint32_t first = rd(d_tile_ps + f), end = rd(d_tile_ps + f + 1);
        if (end <= tile_base || first >= tile_base + tiles) continue;
        const RetPQ q = rd(d_q + f);
        check_segments(v, q, d_tile_ps, f);
        for (uint32_t t = std::max(first, tile_base); t < std::min<uint64_t>(end, (uint64_t)tile_base + tiles); ++t)
            wr(d_tile_cnt + t, (uint32_t)tile_hits(v, q, d_ids, t - first, now).size());
    }
    return hipSuccess;
}

hipError_t launch_retp_cut(const uint32_t *d_tile_ps, uint32_t nq, const uint32_t *d_tile_cnt, uint32_t limit,
                           uint32_t *d_tile_excl, uint32_t *d_taken, uint64_t *d_next_row, hipStream_t) {
    if (limit == 0) die("a page of no values");
    if (g_next_count != rd(d_tile_ps + nq)) die("the cut before the count pass took every tile");
    for (uint32_t f = 0; f < nq; ++f) {
        const uint32_t first = rd(d_tile_ps + f), end = rd(d_tile_ps + f + 1);
        uint64_t run = 0;
        uint32_t c = first;
        for (; c < end && run < limit; c += RTP_CHUNK)
            for (uint32_t t = c; t < c + RTP_CHUNK && t < end; ++t) {
                wr(d_tile_excl + t, (uint32_t)std::min<uint64_t>(run, limit));
                run += rd(d_tile_cnt + t);
            }
        for (uint32_t t = c; t < end; ++t) wr(d_tile_excl + t, limit);
        wr(d_taken + f, (uint32_t)std::min<uint64_t>(run, limit));
        wr(d_next_row + f, (uint64_t)0);
    }
    return hipSuccess;
}

hipError_t launch_retp_emit(const RetView &v, const RetPQ *d_q, uint32_t nq, const uint32_t *d_ids, const uint32_t *d_tile_ps,
                            uint32_t tile_base, uint32_t tiles, uint64_t now, uint32_t limit, const uint32_t *d_tile_cnt,
                            const uint32_t *d_tile_excl, const uint64_t *d_offs, uint32_t *d_out, uint64_t out_cap,
                            uint64_t *d_next_row, hipStream_t) {
    check_launch(g_next_emit, d_tile_ps, nq, tile_base, tiles);
    for (uint32_t f = 0; f < nq; ++f) {
        const uint32_t first = rd(d_tile_ps + f), end = rd(d_tile_ps + f + 1);
        if (end <= tile_base || first >= tile_base + tiles) continue;
        const RetPQ q = rd(d_q + f);
        const uint64_t off = rd(d_offs + f), taken = rd(d_offs + f + 1) - off;
        for (uint32_t t = std::max(first, tile_base); t < std::min<uint64_t>(end, (uint64_t)tile_base + tiles); ++t) {
            const uint32_t excl = rd(d_tile_excl + t);
            if (excl >= limit || rd(d_tile_cnt + t) == 0) continue;
            const std::vector<uint64_t> rows = tile_hits(v, q, d_ids, t - first, now);
            if (rows.size() != rd(d_tile_cnt + t)) die("the emit pass counts differently");
            for (size_t k = 0; k < rows.size() && excl + k < limit; ++k) {
                if (excl + k >= taken) die("a hit past its filter's list");
                if (off + excl + k < out_cap) wr(d_out + off + excl + k, rd(v.value + rows[k]));
                if (excl + k == (uint64_t)limit - 1) wr(d_next_row + f, rows[k] + 1);
            }
        }
        if (end > tile_base + tiles) continue;
        // the launch with the filter's last tile audits its page against every row of the image
        const std::vector<uint64_t> want = audited(v, q, d_ids, now);
        if (taken != std::min<uint64_t>(want.size(), limit)) die("the page's length is not min(hits in the window, limit)");
        for (uint64_t k = 0; k < taken && off + k < out_cap; ++k)
            if (rd(d_out + off + k) != rd(v.value + want[k])) die("the page is not the window's first hits in scan order");
        if (taken == limit && rd(d_next_row + f) != want[limit - 1] + 1) die("next_row is not the row after the limit-th hit");
        if (taken < limit && rd(d_next_row + f) != 0) die("next_row written by a page that is not full");
    }
    return hipSuccess;
}

}  // namespace tmx
