// tm_retain_page_host.cpp -- tm_retained_match_page, tm_retained_pin and
// tm_retained_unpin (include/tmatch.h, "Match cursors"; kernels:
// tm_retain_page.hip; the store itself: tm_retain_host.cpp).
//
// emqx_retainer_mnesia:match_messages/3 opens a stream on its first call and
// consumes batch_read_number rows of it on every later one
// (emqx_retainer_mnesia.erl:288-304).  Here the stream's position is a row
// index: a filter's rows are visited base range first, tail second, both by
// ascending row, and a cursor is the store's epoch (compactions + 1: rows move
// only at a compaction) above the next row to visit.  The host tokenises and
// narrows exactly as tm_retained_match does, clips both segments by the cursor
// and by the scan window, and leaves every row test and the ranking to the
// device.  One call, one buffer: a filter takes at most `limit` values.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/tmatch.h"
#include "tm_retain_page.h"
#include "tm_retain_store.h"

using namespace tmx;
using namespace tmx_ret;

namespace {

constexpr uint64_t ROW_BITS = 40, ROW_MASK = (1ull << ROW_BITS) - 1;
// values brought back with the offsets, before the one synchronisation, when the page's room is this small;
// a larger room waits for the true total and costs a second copy
constexpr uint64_t EAGER_VALUES = 1u << 18;

// never 0 (BEGIN has none) and never all ones (DONE): 1 .. 2^24 - 2
uint64_t epoch_of(const tm_retained *s) { return s->compactions % 0xFFFFFEull + 1; }
uint64_t cursor_at(const tm_retained *s, uint64_t row) { return epoch_of(s) << ROW_BITS | row; }

enum { B_Q, B_IDS, B_TPS, B_CNT, B_EXCL, B_TAKEN, B_NEXT, B_OFFS, B_SCRATCH, B_OUT };

struct Pending {      // a filter that scans
    uint32_t i;       // its place in the call
    bool clipped;     // the window ended before the tail did
    uint64_t stop;    // ... at this row
};

}  // namespace

extern "C" {

int tm_retained_match_page(tm_retained *s, uint64_t n, const uint8_t *bytes, const uint64_t *offs, uint64_t now,
                           const uint64_t *cursor_in, uint32_t limit, uint64_t scan_rows, uint64_t *out_offs,
                           uint32_t *out_values, uint64_t cap, uint64_t *out_cursor, uint8_t *out_err) {
    if (!s) return fail(TM_EINVAL, "tm_retained_match_page: null handle");
    if (!out_offs || (n && (!bytes || !offs || !out_cursor)) || (cap && !out_values))
        return fail(TM_EINVAL, "tm_retained_match_page: null buffer");
    if (limit == 0) return fail(TM_EINVAL, "tm_retained_match_page: limit is 0");
    if (n > (1u << 24)) return fail(TM_EINVAL, "tm_retained_match_page: more than 2^24 filters in a batch");
    for (uint64_t i = 0; i < n; ++i)
        if (offs[i + 1] < offs[i]) return fail(TM_EINVAL, "tm_retained_match_page: offsets decrease at " + std::to_string(i));
    std::lock_guard<std::mutex> g(s->mu);
    RT_HIP(hipSetDevice(s->device));
    std::vector<Level> lv;
    std::vector<uint32_t> ids, all_ids, tps;
    std::vector<RetPQ> qs;
    std::vector<Pending> pend;
    std::string tmp;
    const uint64_t epoch = epoch_of(s), rows = s->rows();
    uint64_t tiles = 0;
    tps.push_back(0);
    for (uint64_t i = 0; i < n; ++i) {
        if (out_err) out_err[i] = 0;
        out_cursor[i] = TM_RET_CURSOR_DONE;   // until the filter turns out to have rows left
        split_levels(bytes + offs[i], offs[i + 1] - offs[i], lv);
        RetPQ q{};
        bool valid = lv.size() <= (size_t)RT_MAX_LEVELS + 1;
        for (size_t k = 0; valid && k + 1 < lv.size(); ++k) valid = !is_word(lv[k], '#');
        if (!valid) {
            if (out_err) out_err[i] = 2;
            s->no_launch++;
            continue;
        }
        const uint64_t cur = cursor_in ? cursor_in[i] : TM_RET_CURSOR_BEGIN;
        if (cur == TM_RET_CURSOR_DONE) {
            s->no_launch++;
            continue;
        }
        if (cur != TM_RET_CURSOR_BEGIN && (cur >> ROW_BITS) != epoch) {   // rows have moved since it was handed out
            if (out_err) out_err[i] = TM_RET_ESTALE;
            out_cursor[i] = TM_RET_CURSOR_BEGIN;
            s->no_launch++;
            continue;
        }
        const uint64_t start = cur & ROW_MASK;   // (BEGIN: row 0)
        if (is_word(lv.back(), '#')) {
            q.flags |= RQ_HASH;
            lv.pop_back();
        }
        if ((q.flags & RQ_HASH) ? (lv.empty() || is_word(lv[0], '+')) : is_word(lv[0], '+')) q.flags |= RQ_WILD_FIRST;
        q.nlev = (uint32_t)lv.size();
        // its level ids; a literal the dictionary lacks matches no stored topic
        ids.clear();
        bool known = true;
        uint32_t prefix = q.nlev;   // levels before the first wildcard
        for (uint32_t k = 0; known && k < q.nlev; ++k) {
            if (is_word(lv[k], '+')) {
                ids.push_back(RT_PLUS);
                if (prefix == q.nlev) prefix = k;
                continue;
            }
            tmp.assign(reinterpret_cast<const char *>(lv[k].p), lv[k].n);
            auto it = s->dict.find(tmp);
            known = it != s->dict.end();
            if (known) ids.push_back(it->second);
        }
        if (!known) {
            s->no_launch++;
            continue;
        }
        uint64_t lo, hi;
        prefix_range(s, ids.data(), prefix, lo, hi);
        // a wildcard-free filter: the one row that is its prefix range's first (a proper prefix sorts first)
        if (prefix == q.nlev && !(q.flags & RQ_HASH)) hi = lo < hi && s->nlev_of(lo) == q.nlev ? lo + 1 : lo;
        q.skip = prefix;
        // the cursor: below lo it starts at lo, at or past hi (and below base) at the tail
        q.lo = std::min(std::max(lo, start), hi);
        q.hi = hi;
        q.tail_lo = std::min(std::max(s->base, start), rows);
        q.tail_hi = rows;
        // the window: base then tail take at most scan_rows rows
        Pending p{(uint32_t)i, false, 0};
        if (scan_rows && (q.hi - q.lo) + (q.tail_hi - q.tail_lo) > scan_rows) {
            p.clipped = true;
            if (q.hi - q.lo >= scan_rows) {   // (all of the window in the base: a stop at hi is the tail's start)
                q.hi = q.lo + scan_rows;
                q.tail_hi = q.tail_lo;
                p.stop = q.hi;
            } else {
                q.tail_hi = q.tail_lo + (scan_rows - (q.hi - q.lo));
                p.stop = q.tail_hi;
            }
        }
        q.base_tiles = (uint32_t)((q.hi - q.lo + RT_TILE - 1) / RT_TILE);
        q.tail_tiles = (uint32_t)((q.tail_hi - q.tail_lo + RT_TILE - 1) / RT_TILE);
        if (q.base_tiles + q.tail_tiles == 0) {   // no rows at or past the cursor
            s->no_launch++;
            continue;
        }
        tiles += q.base_tiles + q.tail_tiles;
        if (tiles > 0x7FFFFFFFull || all_ids.size() + ids.size() > 0xFFFFFFF0ull)
            return fail(TM_EINVAL, "tm_retained_match_page: the batch scans 2^31 tiles of 256 rows or more in all (the sum "
                                   "over its filters of the rows left in their base range and the tail); split it or set "
                                   "scan_rows");
        q.ids_off = (uint32_t)all_ids.size();
        all_ids.insert(all_ids.end(), ids.begin(), ids.end());
        qs.push_back(q);
        tps.push_back((uint32_t)tiles);
        pend.push_back(p);
    }
    const uint32_t nq = (uint32_t)qs.size();
    std::vector<uint64_t> h_offs(nq + 1, 0), h_next(nq, 0);
    std::vector<uint32_t> h_taken(nq, 0), h_vals;
    const uint64_t room = std::min<uint64_t>(cap, (uint64_t)nq * limit);   // the values the device may write
    const bool eager = room && room <= EAGER_VALUES;
    if (nq) {
        DBuf *b = s->d_page;
        int rc = flush(s);   // (nothing is staged between calls; the view's base and tail are set)
        if (rc == TM_OK) rc = dev_reserve(b[B_Q], nq * sizeof(RetPQ));
        if (rc == TM_OK) rc = dev_reserve(b[B_IDS], std::max<size_t>(all_ids.size(), 1) * 4);
        if (rc == TM_OK) rc = dev_reserve(b[B_TPS], (nq + 1) * 4);
        if (rc == TM_OK) rc = dev_reserve(b[B_CNT], tiles * 4);
        if (rc == TM_OK) rc = dev_reserve(b[B_EXCL], tiles * 4);
        if (rc == TM_OK) rc = dev_reserve(b[B_TAKEN], nq * 4);
        if (rc == TM_OK) rc = dev_reserve(b[B_NEXT], nq * 8);
        if (rc == TM_OK) rc = dev_reserve(b[B_OFFS], (nq + 1) * 8);
        if (rc == TM_OK) rc = dev_reserve(b[B_SCRATCH], nq * 4);
        if (rc == TM_OK) rc = dev_reserve(b[B_OUT], std::max<uint64_t>(room, 1) * 4);
        if (rc != TM_OK) return rc;
        const RetPQ *dq = static_cast<const RetPQ *>(b[B_Q].p);
        const uint32_t *dids = static_cast<const uint32_t *>(b[B_IDS].p), *dtps = static_cast<const uint32_t *>(b[B_TPS].p);
        uint32_t *dcnt = static_cast<uint32_t *>(b[B_CNT].p), *dexcl = static_cast<uint32_t *>(b[B_EXCL].p);
        uint32_t *dtaken = static_cast<uint32_t *>(b[B_TAKEN].p), *dout = static_cast<uint32_t *>(b[B_OUT].p);
        uint64_t *dnext = static_cast<uint64_t *>(b[B_NEXT].p), *doffs = static_cast<uint64_t *>(b[B_OFFS].p);
        RT_HIP(hipMemcpyAsync(b[B_Q].p, qs.data(), nq * sizeof(RetPQ), hipMemcpyHostToDevice, s->stream));
        if (!all_ids.empty())
            RT_HIP(hipMemcpyAsync(b[B_IDS].p, all_ids.data(), all_ids.size() * 4, hipMemcpyHostToDevice, s->stream));
        RT_HIP(hipMemcpyAsync(b[B_TPS].p, tps.data(), (nq + 1) * 4, hipMemcpyHostToDevice, s->stream));
        // a launch takes at most RT_MAX_LAUNCH_TILES tiles (fewer than 2^32 threads): the batch's tiles in runs
        for (uint64_t t0 = 0; t0 < tiles; t0 += RT_MAX_LAUNCH_TILES)
            RT_HIP(launch_retp_count(s->v, dq, nq, dids, dtps, (uint32_t)t0,
                                     (uint32_t)std::min<uint64_t>(RT_MAX_LAUNCH_TILES, tiles - t0), now, dcnt, s->stream));
        RT_HIP(launch_retp_cut(dtps, nq, dcnt, limit, dexcl, dtaken, dnext, s->stream));
        // the offsets are the exclusive sums of `taken` (the launcher also zeroes a word per filter: unused here)
        RT_HIP(launch_ret_offsets(dtaken, nq, doffs, static_cast<uint32_t *>(b[B_SCRATCH].p), s->stream));
        for (uint64_t t0 = 0; t0 < tiles; t0 += RT_MAX_LAUNCH_TILES)
            RT_HIP(launch_retp_emit(s->v, dq, nq, dids, dtps, (uint32_t)t0,
                                    (uint32_t)std::min<uint64_t>(RT_MAX_LAUNCH_TILES, tiles - t0), now, limit, dcnt, dexcl, doffs,
                                    dout, room, dnext, s->stream));
        RT_HIP(hipMemcpyAsync(h_offs.data(), doffs, (nq + 1) * 8, hipMemcpyDeviceToHost, s->stream));
        RT_HIP(hipMemcpyAsync(h_taken.data(), dtaken, nq * 4, hipMemcpyDeviceToHost, s->stream));
        RT_HIP(hipMemcpyAsync(h_next.data(), dnext, nq * 8, hipMemcpyDeviceToHost, s->stream));
        if (eager) {
            h_vals.resize(room);
            RT_HIP(hipMemcpyAsync(h_vals.data(), dout, room * 4, hipMemcpyDeviceToHost, s->stream));
        }
        RT_HIP(hipStreamSynchronize(s->stream));
        s->launches++;
    }
    // the n + 1 offsets and the cursors: a filter that was not scanned has an empty list
    uint64_t k = 0;
    for (uint64_t i = 0; i < n; ++i) {
        out_offs[i] = h_offs[k];
        if (k < nq && pend[k].i == i) {
            if (h_taken[k] == limit) out_cursor[i] = cursor_at(s, h_next[k]);          // the row after the limit-th hit
            else if (pend[k].clipped) out_cursor[i] = cursor_at(s, pend[k].stop);      // a short page, a live cursor
            ++k;                                                                       // (else: the end of the tail, DONE)
        }
    }
    out_offs[n] = h_offs[nq];
    const uint64_t total = h_offs[nq];
    if (total > cap)
        return fail(TM_ECAP, "tm_retained_match_page: " + std::to_string(total) + " values, room for " + std::to_string(cap));
    if (total) {
        if (eager) {
            memcpy(out_values, h_vals.data(), total * 4);
        } else {
            RT_HIP(hipMemcpyAsync(out_values, s->d_page[B_OUT].p, total * 4, hipMemcpyDeviceToHost, s->stream));
            RT_HIP(hipStreamSynchronize(s->stream));
        }
    }
    return TM_OK;
}

int tm_retained_pin(tm_retained *s) {
    if (!s) return fail(TM_EINVAL, "tm_retained_pin: null handle");
    std::lock_guard<std::mutex> g(s->mu);
    s->pins++;
    return TM_OK;
}

int tm_retained_unpin(tm_retained *s) {
    if (!s) return fail(TM_EINVAL, "tm_retained_unpin: null handle");
    std::lock_guard<std::mutex> g(s->mu);
    if (s->pins == 0) return fail(TM_EINVAL, "tm_retained_unpin: the store is not pinned");
    if (--s->pins) return TM_OK;
    if (!s->compact_due && s->tail <= s->tail_max) return TM_OK;
    RT_HIP(hipSetDevice(s->device));
    return compact(s);
}

}  // extern "C"
