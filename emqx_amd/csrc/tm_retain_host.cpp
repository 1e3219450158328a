// tm_retain_host.cpp -- the retained-message store's host side and C ABI
// (include/tmatch.h, "The retained-message store"; kernels: tm_retain.hip).
//
// The host keeps the truth: an exact, refcounted dictionary of level words and
// a mirror of every row (its id sequence, meta, value, expiry) in the device's
// row order.  The device holds the same rows as columns.  A batch of writes is
// applied to the mirror in order, one staged record per row written, and goes
// to the device in one k_ret_apply launch; growth and compaction upload the
// mirror anew.  A match tokenises each filter through the dictionary, finds the
// base range of its literal prefix by binary search in the mirror, and leaves
// every row test to the device.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/tmatch.h"
#include "tm_retain.h"
#include "tm_retain_store.h"   // struct tm_retained and the helpers tm_retain_page_host.cpp shares

using namespace tmx;
using namespace tmx_ret;

namespace {

// row r's id sequence against (ids, n): lexicographic, a proper prefix first
int cmp_seq(const tm_retained *s, uint64_t r, const uint32_t *ids, uint32_t n) {
    const uint32_t *a = s->ids_of(r);
    const uint32_t m = s->nlev_of(r), k = std::min(m, n);
    for (uint32_t i = 0; i < k; ++i)
        if (a[i] != ids[i]) return a[i] < ids[i] ? -1 : 1;
    return m < n ? -1 : m > n ? 1 : 0;
}

std::string seq_key(const uint32_t *ids, uint32_t n) { return std::string(reinterpret_cast<const char *>(ids), (size_t)n * 4); }

// the row that holds this id sequence, live or dead (-1: none)
int64_t find_row(const tm_retained *s, const uint32_t *ids, uint32_t n) {
    uint64_t lo, hi;
    prefix_range(s, ids, n, lo, hi);
    if (lo < hi && s->nlev_of(lo) == n) return (int64_t)lo;   // a proper prefix sorts first
    auto it = s->tail_rows.find(seq_key(ids, n));
    return it == s->tail_rows.end() ? -1 : (int64_t)it->second;
}

uint32_t intern(tm_retained *s, const std::string &w) {
    auto it = s->dict.find(w);
    if (it != s->dict.end()) return it->second;
    uint32_t id;
    if (!s->free_ids.empty()) {
        id = s->free_ids.back();
        s->free_ids.pop_back();
    } else {
        id = (uint32_t)s->refc.size();
        s->refc.push_back(0);
    }
    s->refc[id] = 0;
    s->dict.emplace(w, id);
    return id;
}

void free_view(tm_retained *s) {
    void *ps[] = {s->v.cols, s->v.meta, s->v.value, s->v.expiry, s->v.ovf_off, s->v.ovf};
    for (void *p : ps)
        if (p) (void)hipFree(p);
    const uint64_t b = s->base, t = s->tail;
    s->v = RetView{};
    s->v.base = b;
    s->v.tail = t;
}

uint64_t view_bytes(const RetView &v) { return v.stride * (RT_COLS * 4 + 4 + 4 + 8 + 8) + v.ovf_cap * 4; }

// the mirror to the device, anew: arrays of `cap` rows and `ovf_cap` overflow words; staged writes are dropped
// (the mirror has them)
int upload_all(tm_retained *s, uint64_t cap, uint64_t ovf_cap) {
    const uint64_t n = s->rows();
    // overflow runs are laid out tight, in row order
    uint64_t used = 0;
    for (uint64_t r = 0; r < n; ++r) {
        const uint32_t m = s->nlev_of(r);
        s->h_ovf[r] = used;
        if (m > RT_COLS) used += m - RT_COLS;
    }
    cap = std::max<uint64_t>(cap, std::max<uint64_t>(n, 1));
    ovf_cap = std::max<uint64_t>(ovf_cap, std::max<uint64_t>(used, 1));
    s->ops.clear();
    s->words.clear();
    s->op_of_row.clear();
    free_view(s);
    RetView &v = s->v;
    if (hipMalloc((void **)&v.cols, cap * RT_COLS * 4) != hipSuccess || hipMalloc((void **)&v.meta, cap * 4) != hipSuccess ||
        hipMalloc((void **)&v.value, cap * 4) != hipSuccess || hipMalloc((void **)&v.expiry, cap * 8) != hipSuccess ||
        hipMalloc((void **)&v.ovf_off, cap * 8) != hipSuccess || hipMalloc((void **)&v.ovf, ovf_cap * 4) != hipSuccess) {
        free_view(s);
        return fail(TM_ENOMEM, "tm_retained: no device memory for the row columns");
    }
    v.stride = cap;
    v.ovf_cap = ovf_cap;
    v.base = s->base;
    v.tail = s->tail;
    s->ovf_used = used;
    if (n) {
        std::vector<uint32_t> col(n);
        for (uint32_t l = 0; l < RT_COLS; ++l) {
            for (uint64_t r = 0; r < n; ++r) col[r] = l < s->nlev_of(r) ? s->ids_of(r)[l] : RT_PLUS;
            RT_HIP(hipMemcpy(v.cols + (uint64_t)l * cap, col.data(), n * 4, hipMemcpyHostToDevice));
        }
        RT_HIP(hipMemcpy(v.meta, s->h_meta.data(), n * 4, hipMemcpyHostToDevice));
        RT_HIP(hipMemcpy(v.value, s->h_val.data(), n * 4, hipMemcpyHostToDevice));
        RT_HIP(hipMemcpy(v.expiry, s->h_exp.data(), n * 8, hipMemcpyHostToDevice));
        RT_HIP(hipMemcpy(v.ovf_off, s->h_ovf.data(), n * 8, hipMemcpyHostToDevice));
        if (used) {
            std::vector<uint32_t> ovf(used);
            for (uint64_t r = 0; r < n; ++r) {
                const uint32_t m = s->nlev_of(r);
                if (m > RT_COLS) memcpy(ovf.data() + s->h_ovf[r], s->ids_of(r) + RT_COLS, (size_t)(m - RT_COLS) * 4);
            }
            RT_HIP(hipMemcpy(v.ovf, ovf.data(), used * 4, hipMemcpyHostToDevice));
        }
    }
    return TM_OK;
}

}  // namespace

// the staged writes to the device: two copies and one kernel on the store's stream
int tmx_ret::flush(tm_retained *s) {
    s->v.base = s->base;
    s->v.tail = s->tail;
    if (s->ops.empty()) return TM_OK;
    int rc = dev_reserve(s->d_ops, s->ops.size() * sizeof(RetOp));
    if (rc == TM_OK) rc = dev_reserve(s->d_words, std::max<size_t>(s->words.size(), 1) * 4);
    if (rc != TM_OK) return rc;
    RT_HIP(hipMemcpyAsync(s->d_ops.p, s->ops.data(), s->ops.size() * sizeof(RetOp), hipMemcpyHostToDevice, s->stream));
    if (!s->words.empty())
        RT_HIP(hipMemcpyAsync(s->d_words.p, s->words.data(), s->words.size() * 4, hipMemcpyHostToDevice, s->stream));
    RT_HIP(launch_ret_apply(s->v, static_cast<const RetOp *>(s->d_ops.p), (uint32_t)s->ops.size(),
                            static_cast<const uint32_t *>(s->d_words.p), s->words.size(), s->stream));
    RT_HIP(hipStreamSynchronize(s->stream));   // the staging vectors are reused by the next batch
    s->ops.clear();
    s->words.clear();
    s->op_of_row.clear();
    return TM_OK;
}

namespace {

// row r's meta, value and expiry have changed in the mirror
void stage_set(tm_retained *s, uint32_t r) {
    auto it = s->op_of_row.find(r);
    if (it == s->op_of_row.end()) {
        it = s->op_of_row.emplace(r, (uint32_t)s->ops.size()).first;
        s->ops.push_back(RetOp{r, 0, 0, 0, 0, 0, 0});
    }
    RetOp &op = s->ops[it->second];
    op.meta = s->h_meta[r];
    op.value = s->h_val[r];
    op.expiry = s->h_exp[r];
}

uint32_t meta_of(uint32_t nlev, bool dollar, uint64_t expiry) {
    return nlev | RT_LIVE | (dollar ? RT_DOLLAR : 0) | (expiry ? RT_HAS_EXPIRY : 0) | (nlev > RT_COLS ? RT_HAS_OVF : 0);
}

void kill_row(tm_retained *s, uint32_t r) {
    s->h_meta[r] &= ~RT_LIVE;
    const uint32_t *ids = s->ids_of(r);
    for (uint32_t i = 0, m = s->nlev_of(r); i < m; ++i) s->refc[ids[i]]--;
    s->live--;
    stage_set(s, r);
}

}  // namespace

// dead rows dropped, the tail merged into the sorted base, unused dictionary ids freed, everything uploaded
int tmx_ret::compact(tm_retained *s) {
    const uint64_t n = s->rows();
    std::vector<uint32_t> order;   // live tail rows, sorted by id sequence
    for (uint64_t r = s->base; r < n; ++r)
        if (s->h_meta[r] & RT_LIVE) order.push_back((uint32_t)r);
    std::sort(order.begin(), order.end(),
              [&](uint32_t a, uint32_t b) { return cmp_seq(s, a, s->ids_of(b), s->nlev_of(b)) < 0; });
    std::vector<uint32_t> ids, meta, val;
    std::vector<uint64_t> off, exp;
    ids.reserve(s->h_ids.size());
    off.reserve(s->live + 1);
    meta.reserve(s->live);
    val.reserve(s->live);
    exp.reserve(s->live);
    off.push_back(0);
    auto take = [&](uint64_t r) {
        ids.insert(ids.end(), s->ids_of(r), s->ids_of(r) + s->nlev_of(r));
        off.push_back(ids.size());
        meta.push_back(s->h_meta[r]);
        val.push_back(s->h_val[r]);
        exp.push_back(s->h_exp[r]);
    };
    uint64_t a = 0;
    size_t b = 0;
    for (;;) {
        while (a < s->base && !(s->h_meta[a] & RT_LIVE)) ++a;
        if (a == s->base && b == order.size()) break;
        if (b == order.size() || (a < s->base && cmp_seq(s, a, s->ids_of(order[b]), s->nlev_of(order[b])) < 0)) take(a++);
        else take(order[b++]);
    }
    s->h_ids.swap(ids);
    s->h_off.swap(off);
    s->h_meta.swap(meta);
    s->h_val.swap(val);
    s->h_exp.swap(exp);
    s->base = s->h_meta.size();
    s->tail = 0;
    s->h_ovf.assign(s->base, 0);
    s->tail_rows.clear();
    for (auto it = s->dict.begin(); it != s->dict.end();) {
        if (s->refc[it->second] == 0) {
            s->free_ids.push_back(it->second);
            it = s->dict.erase(it);
        } else {
            ++it;
        }
    }
    s->compactions++;
    s->compact_due = false;
    return upload_all(s, s->v.stride, s->v.ovf_cap);
}

namespace {

// after a batch of writes: past tail_max the store compacts, unless a match cursor has pinned it (row indices
// then stay put, and the unpin that brings the count to 0 compacts); else the staged writes go out
int settle(tm_retained *s) { return s->tail > s->tail_max && s->pins == 0 ? compact(s) : flush(s); }

}  // namespace

extern "C" {

const char *tm_retained_last_error(tm_retained *) { return g_ret_error.c_str(); }

int tm_retained_create(int device, const tm_retained_opts *opts, tm_retained **out) {
    if (!out) return fail(TM_EINVAL, "tm_retained_create: out is NULL");
    *out = nullptr;
    tm_retained *s = new (std::nothrow) tm_retained;
    if (!s) return fail(TM_ENOMEM, "tm_retained_create: out of host memory");
    if (device < 0 && hipGetDevice(&device) != hipSuccess) {
        delete s;
        return fail(TM_EDEVICE, "tm_retained_create: no current HIP device");
    }
    s->device = device;
    if (opts && opts->tail_max) s->tail_max = opts->tail_max;
    const uint64_t cap = opts && opts->initial_rows ? opts->initial_rows : 1024;
    s->h_off.push_back(0);
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete s;
        return fail(TM_EDEVICE, std::string("tm_retained_create: ") + hipGetErrorString(e));
    }
    const int rc = upload_all(s, cap, 64);
    if (rc != TM_OK) {
        tm_retained_destroy(s);
        return rc;
    }
    *out = s;
    return TM_OK;
}

int tm_retained_destroy(tm_retained *s) {
    if (!s) return fail(TM_EINVAL, "tm_retained_destroy: null handle");
    (void)hipSetDevice(s->device);
    if (s->stream) {
        (void)hipStreamSynchronize(s->stream);
        (void)hipStreamDestroy(s->stream);
    }
    free_view(s);
    for (DBuf *b : {&s->d_ops, &s->d_words, &s->d_q, &s->d_ids, &s->d_tps, &s->d_counts, &s->d_offs, &s->d_cursor, &s->d_out})
        dev_release(*b);
    for (DBuf &b : s->d_page) dev_release(b);
    delete s;
    return TM_OK;
}

int tm_retained_put(tm_retained *s, uint64_t n, const uint8_t *bytes, const uint64_t *offs, const uint32_t *values,
                    const uint64_t *expiry, uint8_t *out_code) {
    if (!s) return fail(TM_EINVAL, "tm_retained_put: null handle");
    if (n && (!bytes || !offs || !values)) return fail(TM_EINVAL, "tm_retained_put: null buffer");
    for (uint64_t i = 0; i < n; ++i)
        if (offs[i + 1] < offs[i]) return fail(TM_EINVAL, "tm_retained_put: offsets decrease at " + std::to_string(i));
    std::lock_guard<std::mutex> g(s->mu);
    RT_HIP(hipSetDevice(s->device));
    std::vector<Level> lv;
    std::vector<uint32_t> ids;
    std::string tmp;
    for (uint64_t i = 0; i < n; ++i) {
        const uint8_t *p = bytes + offs[i];
        const size_t len = offs[i + 1] - offs[i];
        split_levels(p, len, lv);
        bool valid = len > 0 && lv.size() <= RT_MAX_LEVELS;
        for (size_t k = 0; valid && k < lv.size(); ++k) valid = !is_word(lv[k], '+') && !is_word(lv[k], '#');
        if (!valid) {
            if (out_code) out_code[i] = 2;
            continue;
        }
        const uint32_t m = (uint32_t)lv.size();
        const uint64_t exp = expiry ? expiry[i] : 0;
        const int64_t found = lookup_ids(s, lv, ids, tmp) ? find_row(s, ids.data(), m) : -1;
        if (found >= 0) {
            const uint32_t r = (uint32_t)found;
            const bool was_live = (s->h_meta[r] & RT_LIVE) != 0;
            if (!was_live) {   // a deleted row not yet compacted away: it lives again where it is
                for (uint32_t id : ids) s->refc[id]++;
                s->live++;
            }
            s->h_meta[r] = meta_of(m, p[0] == '$', exp);
            s->h_val[r] = values[i];
            s->h_exp[r] = exp;
            stage_set(s, r);
            if (out_code) out_code[i] = was_live ? 0 : 1;
            continue;
        }
        // a new row at the end of the tail
        const uint64_t r = s->rows();
        if (r >= 0xFFFFFFF0ull) return fail(TM_ENOMEM, "tm_retained_put: the store holds 2^32 - 16 rows");
        const uint64_t extra = m > RT_COLS ? m - RT_COLS : 0;
        if (r + 1 > s->v.stride || s->ovf_used + extra > s->v.ovf_cap) {
            const uint64_t cap = r + 1 > s->v.stride ? std::max<uint64_t>(s->v.stride * 2, r + 1) : s->v.stride;
            const uint64_t oc = s->ovf_used + extra > s->v.ovf_cap ? std::max<uint64_t>(s->v.ovf_cap * 2, s->ovf_used + extra)
                                                                   : s->v.ovf_cap;
            const int rc = upload_all(s, cap, oc);
            if (rc != TM_OK) return rc;
            s->growths++;
        }
        ids.clear();
        for (const Level &l : lv) {
            tmp.assign(reinterpret_cast<const char *>(l.p), l.n);
            const uint32_t id = intern(s, tmp);
            s->refc[id]++;
            ids.push_back(id);
        }
        s->h_ids.insert(s->h_ids.end(), ids.begin(), ids.end());
        s->h_off.push_back(s->h_ids.size());
        s->h_meta.push_back(meta_of(m, p[0] == '$', exp));
        s->h_val.push_back(values[i]);
        s->h_exp.push_back(exp);
        s->h_ovf.push_back(s->ovf_used);
        s->tail_rows.emplace(seq_key(ids.data(), m), (uint32_t)r);
        s->op_of_row.emplace((uint32_t)r, (uint32_t)s->ops.size());
        s->ops.push_back(RetOp{(uint32_t)r, s->h_meta[r], values[i], m, exp, s->ovf_used, (uint64_t)s->words.size()});
        s->words.insert(s->words.end(), ids.begin(), ids.end());
        s->ovf_used += extra;
        s->tail++;
        s->live++;
        if (out_code) out_code[i] = 1;
    }
    return settle(s);
}

int tm_retained_delete(tm_retained *s, uint64_t n, const uint8_t *bytes, const uint64_t *offs, uint8_t *out_found) {
    if (!s) return fail(TM_EINVAL, "tm_retained_delete: null handle");
    if (n && (!bytes || !offs)) return fail(TM_EINVAL, "tm_retained_delete: null buffer");
    for (uint64_t i = 0; i < n; ++i)
        if (offs[i + 1] < offs[i]) return fail(TM_EINVAL, "tm_retained_delete: offsets decrease at " + std::to_string(i));
    std::lock_guard<std::mutex> g(s->mu);
    RT_HIP(hipSetDevice(s->device));
    std::vector<Level> lv;
    std::vector<uint32_t> ids;
    std::string tmp;
    for (uint64_t i = 0; i < n; ++i) {
        split_levels(bytes + offs[i], offs[i + 1] - offs[i], lv);
        const int64_t r = lookup_ids(s, lv, ids, tmp) ? find_row(s, ids.data(), (uint32_t)ids.size()) : -1;
        const bool found = r >= 0 && (s->h_meta[r] & RT_LIVE);
        if (found) kill_row(s, (uint32_t)r);
        if (out_found) out_found[i] = found;
    }
    return settle(s);
}

int tm_retained_get(tm_retained *s, uint64_t n, const uint8_t *bytes, const uint64_t *offs, uint64_t now,
                    uint32_t *out_value, uint8_t *out_found) {
    if (!s) return fail(TM_EINVAL, "tm_retained_get: null handle");
    if (n && (!bytes || !offs || !out_value || !out_found)) return fail(TM_EINVAL, "tm_retained_get: null buffer");
    for (uint64_t i = 0; i < n; ++i)
        if (offs[i + 1] < offs[i]) return fail(TM_EINVAL, "tm_retained_get: offsets decrease at " + std::to_string(i));
    std::lock_guard<std::mutex> g(s->mu);
    std::vector<Level> lv;
    std::vector<uint32_t> ids;
    std::string tmp;
    for (uint64_t i = 0; i < n; ++i) {
        split_levels(bytes + offs[i], offs[i + 1] - offs[i], lv);
        const int64_t r = lookup_ids(s, lv, ids, tmp) ? find_row(s, ids.data(), (uint32_t)ids.size()) : -1;
        // the read path's rule: >= (emqx_retainer_mnesia.erl:510)
        const bool found = r >= 0 && (s->h_meta[r] & RT_LIVE) && (s->h_exp[r] == 0 || s->h_exp[r] >= now);
        out_found[i] = found;
        out_value[i] = found ? s->h_val[r] : 0;
    }
    return TM_OK;
}

int tm_retained_match(tm_retained *s, uint64_t n, const uint8_t *bytes, const uint64_t *offs, uint64_t now,
                      uint64_t *out_offs, uint32_t *out_values, uint64_t cap, uint8_t *out_err) {
    if (!s) return fail(TM_EINVAL, "tm_retained_match: null handle");
    if (!out_offs || (n && (!bytes || !offs)) || (cap && !out_values)) return fail(TM_EINVAL, "tm_retained_match: null buffer");
    if (n > (1u << 24)) return fail(TM_EINVAL, "tm_retained_match: more than 2^24 filters in a batch");
    for (uint64_t i = 0; i < n; ++i)
        if (offs[i + 1] < offs[i]) return fail(TM_EINVAL, "tm_retained_match: offsets decrease at " + std::to_string(i));
    std::lock_guard<std::mutex> g(s->mu);
    RT_HIP(hipSetDevice(s->device));
    std::vector<Level> lv;
    std::vector<uint32_t> ids, all_ids, tps, which;
    std::vector<RetQ> qs;
    std::string tmp;
    const uint32_t tail_tiles = (uint32_t)((s->tail + RT_TILE - 1) / RT_TILE);
    uint64_t tiles = 0;
    tps.push_back(0);
    for (uint64_t i = 0; i < n; ++i) {
        if (out_err) out_err[i] = 0;
        split_levels(bytes + offs[i], offs[i + 1] - offs[i], lv);
        RetQ q{};
        bool valid = lv.size() <= (size_t)RT_MAX_LEVELS + 1;
        for (size_t k = 0; valid && k + 1 < lv.size(); ++k) valid = !is_word(lv[k], '#');
        if (!valid) {
            if (out_err) out_err[i] = 2;
            s->no_launch++;
            continue;
        }
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
        prefix_range(s, ids.data(), prefix, q.lo, q.hi);
        // a wildcard-free filter: the one row that is its prefix range's first (a proper prefix sorts first)
        if (prefix == q.nlev && !(q.flags & RQ_HASH)) q.hi = q.lo < q.hi && s->nlev_of(q.lo) == q.nlev ? q.lo + 1 : q.lo;
        q.skip = prefix;
        q.base_tiles = (uint32_t)((q.hi - q.lo + RT_TILE - 1) / RT_TILE);
        if (q.base_tiles + tail_tiles == 0) {
            s->no_launch++;
            continue;
        }
        tiles += q.base_tiles + tail_tiles;
        if (tiles > 0x7FFFFFFFull || all_ids.size() + ids.size() > 0xFFFFFFF0ull)
            return fail(TM_EINVAL, "tm_retained_match: the batch scans 2^31 tiles of 256 rows or more in all (the sum over "
                                   "its filters of their base range and the tail); split it");
        q.ids_off = (uint32_t)all_ids.size();
        all_ids.insert(all_ids.end(), ids.begin(), ids.end());
        qs.push_back(q);
        tps.push_back((uint32_t)tiles);
        which.push_back((uint32_t)i);
    }
    const uint32_t nq = (uint32_t)qs.size();
    std::vector<uint64_t> d_offs(nq + 1, 0);
    if (nq) {
        int rc = flush(s);   // (nothing is staged between calls; the view's base and tail are set)
        if (rc == TM_OK) rc = dev_reserve(s->d_q, nq * sizeof(RetQ));
        if (rc == TM_OK) rc = dev_reserve(s->d_ids, std::max<size_t>(all_ids.size(), 1) * 4);
        if (rc == TM_OK) rc = dev_reserve(s->d_tps, (nq + 1) * 4);
        if (rc == TM_OK) rc = dev_reserve(s->d_counts, nq * 4);
        if (rc == TM_OK) rc = dev_reserve(s->d_cursor, nq * 4);
        if (rc == TM_OK) rc = dev_reserve(s->d_offs, (nq + 1) * 8);
        if (rc != TM_OK) return rc;
        const RetQ *dq = static_cast<const RetQ *>(s->d_q.p);
        const uint32_t *dids = static_cast<const uint32_t *>(s->d_ids.p), *dtps = static_cast<const uint32_t *>(s->d_tps.p);
        uint32_t *dcounts = static_cast<uint32_t *>(s->d_counts.p), *dcursor = static_cast<uint32_t *>(s->d_cursor.p);
        uint64_t *doffs = static_cast<uint64_t *>(s->d_offs.p);
        RT_HIP(hipMemcpyAsync(s->d_q.p, qs.data(), nq * sizeof(RetQ), hipMemcpyHostToDevice, s->stream));
        if (!all_ids.empty())
            RT_HIP(hipMemcpyAsync(s->d_ids.p, all_ids.data(), all_ids.size() * 4, hipMemcpyHostToDevice, s->stream));
        RT_HIP(hipMemcpyAsync(s->d_tps.p, tps.data(), (nq + 1) * 4, hipMemcpyHostToDevice, s->stream));
        RT_HIP(hipMemsetAsync(dcounts, 0, nq * 4, s->stream));
        // a launch takes at most RT_MAX_LAUNCH_TILES tiles (fewer than 2^32 threads): the batch's tiles in runs
        for (uint64_t t0 = 0; t0 < tiles; t0 += RT_MAX_LAUNCH_TILES)
            RT_HIP(launch_ret_count(s->v, dq, nq, dids, dtps, (uint32_t)t0,
                                    (uint32_t)std::min<uint64_t>(RT_MAX_LAUNCH_TILES, tiles - t0), now, dcounts, s->stream));
        RT_HIP(launch_ret_offsets(dcounts, nq, doffs, dcursor, s->stream));
        RT_HIP(hipMemcpyAsync(d_offs.data(), doffs, (nq + 1) * 8, hipMemcpyDeviceToHost, s->stream));
        RT_HIP(hipStreamSynchronize(s->stream));
        s->launches++;
    }
    // the n + 1 offsets: a filter that was not scanned has an empty list
    uint64_t k = 0;
    for (uint64_t i = 0; i < n; ++i) {
        out_offs[i] = d_offs[k];
        if (k < nq && which[k] == i) ++k;
    }
    out_offs[n] = d_offs[nq];
    const uint64_t total = d_offs[nq];
    if (total > cap) return fail(TM_ECAP, "tm_retained_match: " + std::to_string(total) + " values, room for " + std::to_string(cap));
    if (total) {
        const int rc = dev_reserve(s->d_out, total * 4);
        if (rc != TM_OK) return rc;
        for (uint64_t t0 = 0; t0 < tiles; t0 += RT_MAX_LAUNCH_TILES)
            RT_HIP(launch_ret_emit(s->v, static_cast<const RetQ *>(s->d_q.p), nq, static_cast<const uint32_t *>(s->d_ids.p),
                                   static_cast<const uint32_t *>(s->d_tps.p), (uint32_t)t0,
                                   (uint32_t)std::min<uint64_t>(RT_MAX_LAUNCH_TILES, tiles - t0), now,
                                   static_cast<const uint64_t *>(s->d_offs.p), static_cast<uint32_t *>(s->d_cursor.p),
                                   static_cast<uint32_t *>(s->d_out.p), total, s->stream));
        RT_HIP(hipMemcpyAsync(out_values, s->d_out.p, total * 4, hipMemcpyDeviceToHost, s->stream));
        RT_HIP(hipStreamSynchronize(s->stream));
    }
    return TM_OK;
}

int tm_retained_expire(tm_retained *s, uint64_t deadline, uint64_t limit, uint32_t *out_values, uint64_t cap,
                       uint64_t *out_n, int *out_complete) {
    if (!s) return fail(TM_EINVAL, "tm_retained_expire: null handle");
    if (!out_n || !out_complete || (cap && !out_values)) return fail(TM_EINVAL, "tm_retained_expire: null buffer");
    std::lock_guard<std::mutex> g(s->mu);
    RT_HIP(hipSetDevice(s->device));
    uint64_t room = limit ? limit : ~0ull, done = 0;
    if (out_values) room = std::min(room, cap);
    int complete = 1;
    for (uint64_t r = 0, n = s->rows(); r < n; ++r) {
        if (!(s->h_meta[r] & RT_LIVE) || s->h_exp[r] == 0 || s->h_exp[r] >= deadline) continue;
        if (done == room) {   // stopped by the limit with expired rows left
            complete = 0;
            break;
        }
        if (out_values) out_values[done] = s->h_val[r];
        kill_row(s, (uint32_t)r);
        ++done;
    }
    // Complete is "the stream ended before `limit` rows were taken" (emqx_utils_stream:fold/4 hands back a
    // stream, not [], once it has folded N elements: :266-267), so exactly `limit` expired rows is not complete
    if (limit && done == limit) complete = 0;
    *out_n = done;
    *out_complete = complete;
    return settle(s);
}

int tm_retained_compact(tm_retained *s) {
    if (!s) return fail(TM_EINVAL, "tm_retained_compact: null handle");
    std::lock_guard<std::mutex> g(s->mu);
    RT_HIP(hipSetDevice(s->device));
    if (s->pins) {   // pinned: the compaction becomes due (tm_retained_unpin)
        s->compact_due = true;
        return TM_OK;
    }
    return compact(s);
}

int tm_retained_stats(tm_retained *s, tm_retained_stats_t *out) {
    if (!s || !out) return fail(TM_EINVAL, "tm_retained_stats: null argument");
    std::lock_guard<std::mutex> g(s->mu);
    out->live_rows = s->live;
    out->base_rows = s->base;
    out->tail_rows = s->tail;
    out->dead_rows = s->rows() - s->live;
    out->words = s->dict.size();
    out->compactions = s->compactions;
    out->growths = s->growths;
    out->match_launches = s->launches;
    out->no_launch_filters = s->no_launch;
    uint64_t bytes = view_bytes(s->v);
    for (const DBuf *b : {&s->d_ops, &s->d_words, &s->d_q, &s->d_ids, &s->d_tps, &s->d_counts, &s->d_offs, &s->d_cursor, &s->d_out})
        bytes += b->bytes;
    for (const DBuf &b : s->d_page) bytes += b.bytes;
    out->device_bytes = bytes;
    out->rt_cols = RT_COLS;
    out->rt_tile = RT_TILE;
    return TM_OK;
}

}  // extern "C"
