// tm_retain_store.h -- the retained store's handle and the host helpers its two
// host files share (tm_retain_host.cpp: the store and tm_retained_match;
// tm_retain_page_host.cpp: tm_retained_match_page, pin and unpin).  Internal:
// include/tmatch.h is the interface.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/tmatch.h"
#include "tm_retain.h"

namespace tmx_ret {

inline thread_local std::string g_ret_error;

inline int fail(int code, const std::string &msg) {
    g_ret_error = msg;
    return code;
}

#define RT_HIP(x)                                                                          \
    do {                                                                                   \
        hipError_t e_ = (x);                                                               \
        if (e_ != hipSuccess) return tmx_ret::fail(TM_EDEVICE, std::string(#x ": ") + hipGetErrorString(e_)); \
    } while (0)

struct DBuf {   // a device buffer that only grows
    void *p = nullptr;
    size_t bytes = 0;
};

struct Level {
    const uint8_t *p;
    size_t n;
};

inline void split_levels(const uint8_t *p, size_t n, std::vector<Level> &out) {
    out.clear();
    size_t b = 0;
    for (size_t i = 0; i <= n; ++i)
        if (i == n || p[i] == '/') {
            out.push_back({p + b, i - b});
            b = i + 1;
        }
}

inline bool is_word(const Level &l, char c) { return l.n == 1 && l.p[0] == (uint8_t)c; }

}  // namespace tmx_ret

struct tm_retained {
    std::mutex mu;
    int device = 0;
    hipStream_t stream = nullptr;
    uint32_t tail_max = 4096;

    // the dictionary: exact (keyed by the word's bytes), counted by live rows
    std::unordered_map<std::string, uint32_t> dict;
    std::vector<uint32_t> refc;
    std::vector<uint32_t> free_ids;

    // the mirror, in the device's row order
    std::vector<uint32_t> h_ids;      // every row's level ids, row-major
    std::vector<uint64_t> h_off;      // rows + 1
    std::vector<uint32_t> h_meta, h_val;
    std::vector<uint64_t> h_exp, h_ovf;
    uint64_t base = 0, tail = 0, live = 0, ovf_used = 0;
    std::unordered_map<std::string, uint32_t> tail_rows;   // id sequence (bytes) -> row, tail rows only

    // the device
    tmx::RetView v{};
    tmx_ret::DBuf d_ops, d_words, d_q, d_ids, d_tps, d_counts, d_offs, d_cursor, d_out;
    // ... and tm_retained_match_page's batch buffers: descriptors, ids, tile prefix sums, per-tile counts and
    // exclusive counts, per-filter taken / next row / offsets, launch_ret_offsets' cursor words, the values
    tmx_ret::DBuf d_page[10];
    std::vector<tmx::RetOp> ops;
    std::vector<uint32_t> words;
    std::unordered_map<uint32_t, uint32_t> op_of_row;

    uint64_t compactions = 0, growths = 0, launches = 0, no_launch = 0;

    // match cursors: while a holder has pinned the store it does not compact (row indices stay put)
    uint64_t pins = 0;
    bool compact_due = false;   // tm_retained_compact was asked for under a pin

    uint64_t rows() const { return base + tail; }
    const uint32_t *ids_of(uint64_t r) const { return h_ids.data() + h_off[r]; }
    uint32_t nlev_of(uint64_t r) const { return (uint32_t)(h_off[r + 1] - h_off[r]); }
};

namespace tmx_ret {

// row r against the prefix (ids, p): 0 when the row starts with it
inline int cmp_prefix(const tm_retained *s, uint64_t r, const uint32_t *ids, uint32_t p) {
    const uint32_t *a = s->ids_of(r);
    const uint32_t m = s->nlev_of(r), k = std::min(m, p);
    for (uint32_t i = 0; i < k; ++i)
        if (a[i] != ids[i]) return a[i] < ids[i] ? -1 : 1;
    return m < p ? -1 : 0;
}

// the base rows [lo, hi) that start with (ids, p)
inline void prefix_range(const tm_retained *s, const uint32_t *ids, uint32_t p, uint64_t &lo, uint64_t &hi) {
    uint64_t a = 0, b = s->base;
    while (a < b) {
        const uint64_t m = a + (b - a) / 2;
        if (cmp_prefix(s, m, ids, p) < 0) a = m + 1; else b = m;
    }
    lo = a;
    b = s->base;
    while (a < b) {
        const uint64_t m = a + (b - a) / 2;
        if (cmp_prefix(s, m, ids, p) <= 0) a = m + 1; else b = m;
    }
    hi = a;
}

// the ids of known words; false when a word is not in the dictionary
inline bool lookup_ids(const tm_retained *s, const std::vector<Level> &lv, std::vector<uint32_t> &ids, std::string &tmp) {
    ids.clear();
    for (const Level &l : lv) {
        tmp.assign(reinterpret_cast<const char *>(l.p), l.n);
        auto it = s->dict.find(tmp);
        if (it == s->dict.end()) return false;
        ids.push_back(it->second);
    }
    return true;
}

inline int dev_reserve(DBuf &b, size_t bytes) {
    if (bytes <= b.bytes) return TM_OK;
    size_t want = std::max(bytes, b.bytes * 2);
    if (b.p) RT_HIP(hipFree(b.p));
    b.p = nullptr;
    b.bytes = 0;
    if (hipMalloc(&b.p, want) != hipSuccess) return fail(TM_ENOMEM, "tm_retained: no device memory for a batch buffer");
    b.bytes = want;
    return TM_OK;
}

inline void dev_release(DBuf &b) {
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.bytes = 0;
}

// (tm_retain_host.cpp) the staged writes to the device; dead rows dropped, the tail merged, everything uploaded.
// Both with the store's mutex held and its device current.
int flush(tm_retained *s);
int compact(tm_retained *s);

}  // namespace tmx_ret
