// fake_retain_launch.cpp -- the four tmx::launch_ret_* symbols tm_retain_host.cpp
// links against, in plain C++ over the CPU device fake (tests/host_cpu/fake_hip.cpp).
//
// launch_ret_apply is k_ret_apply's definition.  The match launchers do not
// trust what the host promises: for every filter they test EVERY row of the
// image, all levels from the first, with a plain restatement of
// emqx_topic:match/2 over ids, and abort unless that set equals (a) the same
// test restricted to the segments the filter was handed (a matching row outside
// its prefix range or missing from the tail is caught) and (b) what the kernel
// computes: only the segments' rows, only the levels from `skip` on (a prefix
// range whose rows do not all carry the prefix is caught).  A batch's tiles come
// in launches of at most RT_MAX_LAUNCH_TILES, each with its first tile: a launch
// of 2^32 threads or more, a gap between launches or a tile past the batch is
// refused, and what the launches find tile by tile must add up to the audited
// list.  Every word read or written is checked against the allocation that holds
// it (fake_hip_room).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../emqx_amd/csrc/tm_retain.h"

extern "C" size_t fake_hip_room(const void *p);

namespace {

[[noreturn]] void die(const char *what) {
    fprintf(stderr, "fake_retain_launch: %s\n", what);
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

uint32_t level_id(const tmx::RetView &v, uint64_t row, uint32_t l) {
    using namespace tmx;
    if (l < RT_COLS) return rd(v.cols + (uint64_t)l * v.stride + row);
    if (!(rd(v.meta + row) & RT_HAS_OVF)) die("a level past the columns of a row without overflow");
    const uint64_t at = rd(v.ovf_off + row) + (l - RT_COLS);
    if (at >= v.ovf_cap) die("an overflow run past the array");
    return rd(v.ovf + at);
}

// emqx_topic:match/2 over ids plus the match path's expiry rule, levels `from` .. (from == 0: the restatement)
bool row_matches(const tmx::RetView &v, const tmx::RetQ &q, const uint32_t *ids, uint64_t row, uint32_t from, uint64_t now) {
    using namespace tmx;
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

// the rows filter q hits, audited as the header says
std::vector<uint64_t> hits_of(const tmx::RetView &v, const tmx::RetQ *qs, uint32_t f, const uint32_t *ids, const uint32_t *tps,
                              uint64_t now) {
    using namespace tmx;
    const RetQ q = rd(qs + f);
    const uint64_t n = v.base + v.tail;
    if (n > v.stride) die("more rows than the columns hold");
    if (q.lo > q.hi || q.hi > v.base) die("a base range outside the base");
    const uint32_t tail_tiles = (uint32_t)((v.tail + RT_TILE - 1) / RT_TILE);
    if (q.base_tiles != (q.hi - q.lo + RT_TILE - 1) / RT_TILE) die("base_tiles is not its range's tile count");
    if (rd(tps + f + 1) - rd(tps + f) != q.base_tiles + tail_tiles) die("the tile prefix sums disagree with the segments");
    if (q.skip > q.nlev) die("more prefix levels than levels");
    std::vector<uint64_t> all, seg, kern;
    for (uint64_t r = 0; r < n; ++r) {
        const bool in_base = r >= q.lo && r < q.hi, in_tail = r >= v.base;
        const bool m = row_matches(v, q, ids, r, 0, now);
        if (m) all.push_back(r);
        if (m && (in_base || in_tail)) seg.push_back(r);
        if ((in_base && row_matches(v, q, ids, r, q.skip, now)) || (in_tail && m)) kern.push_back(r);
    }
    if (all != seg) die("a matching row lies outside the segments its filter was handed");
    if (all != kern) die("the kernel's test (levels past the prefix only) differs from the full test");
    return all;
}

// a launch of k_ret_rows: fewer than 2^32 threads, at most RT_MAX_LAUNCH_TILES tiles, and the batch's launches take
// its tiles in order without a gap
uint64_t g_next_count = 0, g_next_emit = 0;

void check_launch(uint64_t &next, const uint32_t *tps, uint32_t nq, uint32_t tile_base, uint32_t tiles) {
    using namespace tmx;
    if ((uint64_t)tiles * RT_TILE >= (1ull << 32)) die("a launch of 2^32 threads or more");
    if (tiles > RT_MAX_LAUNCH_TILES || tiles == 0) die("a launch of no tiles, or of more than RT_MAX_LAUNCH_TILES");
    if (rd(tps) != 0) die("the tile prefix sums do not start at 0");
    const uint64_t total = rd(tps + nq);
    if (tile_base != 0 && tile_base != next) die("a batch's launches leave a gap or overlap");
    if ((uint64_t)tile_base + tiles > total) die("a launch past the batch's tiles");
    if ((uint64_t)tile_base + tiles < total && tiles != RT_MAX_LAUNCH_TILES) die("a short launch that is not the batch's last");
    next = (uint64_t)tile_base + tiles;
}

// what k_ret_rows finds for filter f in the tiles [tile_base, tile_base + tiles) of the batch
std::vector<uint64_t> launch_hits(const tmx::RetView &v, const tmx::RetQ *qs, uint32_t f, const uint32_t *ids, const uint32_t *tps,
                                  uint32_t tile_base, uint32_t tiles, uint64_t now) {
    using namespace tmx;
    const RetQ q = rd(qs + f);
    const uint64_t a = std::max<uint64_t>(rd(tps + f), tile_base), b = std::min<uint64_t>(rd(tps + f + 1), (uint64_t)tile_base + tiles);
    std::vector<uint64_t> out;
    for (uint64_t tile = a; tile < b; ++tile) {
        const uint64_t t = tile - rd(tps + f);
        const bool base = t < q.base_tiles;
        const uint64_t row0 = base ? q.lo + t * RT_TILE : v.base + (t - q.base_tiles) * RT_TILE;
        const uint64_t end = base ? q.hi : v.base + v.tail;
        for (uint64_t r = row0; r < row0 + RT_TILE && r < end; ++r)
            if (row_matches(v, q, ids, r, base ? q.skip : 0, now)) out.push_back(r);
    }
    return out;
}

}  // namespace

namespace tmx {

hipError_t launch_ret_apply(const RetView &v, const RetOp *d_ops, uint32_t n_ops, const uint32_t *d_words, uint64_t n_words,
                            hipStream_t) {
    std::vector<char> seen(v.stride, 0);
    for (uint32_t i = 0; i < n_ops; ++i) {
        const RetOp op = rd(d_ops + i);
        if (op.row >= v.stride) die("k_ret_apply: a row past the columns");
        if (seen[op.row]++) die("k_ret_apply: two writes of one row in one launch");
        if (op.words_off + op.nwords > n_words) die("k_ret_apply: level ids past the staged words");
        for (uint32_t l = 0; l < op.nwords; ++l) {
            const uint32_t w = rd(d_words + op.words_off + l);
            if (l < RT_COLS) {
                wr(v.cols + (uint64_t)l * v.stride + op.row, w);
            } else {
                if (op.ovf_off + (l - RT_COLS) >= v.ovf_cap) die("k_ret_apply: an overflow run past the array");
                wr(v.ovf + op.ovf_off + (l - RT_COLS), w);
            }
        }
        if (op.nwords > RT_COLS) wr(v.ovf_off + op.row, op.ovf_off);
        wr(v.value + op.row, op.value);
        wr(v.expiry + op.row, op.expiry);
        wr(v.meta + op.row, op.meta);
    }
    return hipSuccess;
}

hipError_t launch_ret_count(const RetView &v, const RetQ *d_q, uint32_t nq, const uint32_t *d_ids, const uint32_t *d_tile_ps,
                            uint32_t tile_base, uint32_t tiles, uint64_t now, uint32_t *d_counts, hipStream_t) {
    check_launch(g_next_count, d_tile_ps, nq, tile_base, tiles);
    for (uint32_t f = 0; f < nq; ++f) {
        const uint32_t first = rd(d_tile_ps + f), end = rd(d_tile_ps + f + 1);
        if (end <= tile_base || first >= tile_base + tiles) continue;
        if (first >= tile_base && rd(d_counts + f) != 0) die("a count that was not zeroed");
        wr(d_counts + f, rd(d_counts + f) + (uint32_t)launch_hits(v, d_q, f, d_ids, d_tile_ps, tile_base, tiles, now).size());
        // the launch with the filter's last tile audits it: every row of the image, against what the launches added up
        if (end <= tile_base + tiles && rd(d_counts + f) != hits_of(v, d_q, f, d_ids, d_tile_ps, now).size())
            die("the launches' counts do not add up to the audited list");
    }
    return hipSuccess;
}

hipError_t launch_ret_offsets(const uint32_t *d_counts, uint32_t nq, uint64_t *d_offs, uint32_t *d_cursor, hipStream_t) {
    uint64_t run = 0;
    for (uint32_t f = 0; f < nq; ++f) {
        wr(d_offs + f, run);
        run += rd(d_counts + f);
        wr(d_cursor + f, 0u);
    }
    wr(d_offs + nq, run);
    return hipSuccess;
}

hipError_t launch_ret_emit(const RetView &v, const RetQ *d_q, uint32_t nq, const uint32_t *d_ids, const uint32_t *d_tile_ps,
                           uint32_t tile_base, uint32_t tiles, uint64_t now, const uint64_t *d_offs, uint32_t *d_cursor,
                           uint32_t *d_out, uint64_t out_cap, hipStream_t) {
    check_launch(g_next_emit, d_tile_ps, nq, tile_base, tiles);
    for (uint32_t f = 0; f < nq; ++f) {
        const uint32_t first = rd(d_tile_ps + f), end = rd(d_tile_ps + f + 1);
        if (end <= tile_base || first >= tile_base + tiles) continue;
        if (first >= tile_base && rd(d_cursor + f) != 0) die("a cursor that was not zeroed");
        const std::vector<uint64_t> rows = launch_hits(v, d_q, f, d_ids, d_tile_ps, tile_base, tiles, now);
        // from the back: the order within a list is unspecified, and nobody may rely on the scan's
        for (size_t k = 0; k < rows.size(); ++k) {
            const uint64_t pos = rd(d_offs + f) + rd(d_cursor + f) + k;
            if (pos >= out_cap || pos >= rd(d_offs + f + 1)) die("a hit past its filter's list or the output's capacity");
            wr(d_out + pos, rd(v.value + rows[rows.size() - 1 - k]));
        }
        wr(d_cursor + f, rd(d_cursor + f) + (uint32_t)rows.size());
        if (end <= tile_base + tiles && rd(d_offs + f) + rd(d_cursor + f) != rd(d_offs + f + 1))
            die("the emit pass counts differently");
    }
    return hipSuccess;
}

}  // namespace tmx
