// retain_page_check.cpp -- tm_retained_match_page, tm_retained_pin and
// tm_retained_unpin (emqx_amd/csrc/tm_retain_page_host.cpp, with the store of
// tm_retain_host.cpp) on the CPU device fake, driven through the public ABI
// (tests/test_retain_page_image_cpu.py).
//
// A model (topic -> value, expiry) and a restatement of emqx_topic:match/2 over
// strings give every expected set; fake_retain_page_launch.cpp audits the image,
// the segments and the scan order of every page.  Every call has canaries around
// out_hit_offsets, out_cursor and out_err and after out_values[cap].  Built with
// -fsanitize=address,undefined.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>
#include <string>
#include <thread>
#include <vector>

#include "../../include/tmatch.h"

extern "C" size_t fake_hip_live_allocs(void);

namespace {

#define CHECK(x)                                                        \
    do {                                                                \
        if (!(x)) {                                                     \
            fprintf(stderr, "retain_page_check: %s:%d: %s\n", __FILE__, __LINE__, #x); \
            abort();                                                    \
        }                                                               \
    } while (0)

using Strs = std::vector<std::string>;
using Vals = std::vector<uint32_t>;
constexpr uint64_t BEGIN = TM_RET_CURSOR_BEGIN, DONE = TM_RET_CURSOR_DONE, C64 = 0xFEEDFACECAFEBEEFull;
constexpr uint32_t C32 = 0xC0FFEE11u;

Strs split(const std::string &s) {
    Strs out(1);
    for (char c : s)
        if (c == '/') out.emplace_back(); else out.back() += c;
    return out;
}

// emqx_topic:match/2 (emqx_topic.erl:80-116), restated
bool topic_match(const std::string &topic, const std::string &filter) {
    const Strs t = split(topic), f = split(filter);
    if (!topic.empty() && topic[0] == '$' && (f[0] == "+" || f[0] == "#")) return false;
    size_t i = 0;
    for (; i < f.size(); ++i) {
        if (f[i] == "#") return i + 1 == f.size();
        if (i >= t.size()) return false;
        if (f[i] != "+" && f[i] != t[i]) return false;
    }
    return i == t.size();
}

bool valid_filter(const std::string &filter) {
    const Strs f = split(filter);
    for (size_t i = 0; i + 1 < f.size(); ++i)
        if (f[i] == "#") return false;
    return true;
}

struct Row {
    uint32_t value;
    uint64_t expiry;
};

struct Page {
    int rc;
    std::vector<uint64_t> hit, cursor;
    Vals vals;
    std::vector<uint8_t> err;
    Vals list(size_t i) const { return Vals(vals.begin() + hit[i], vals.begin() + std::min<uint64_t>(hit[i + 1], vals.size())); }
};

struct World {
    tm_retained *r = nullptr;
    std::map<std::string, Row> model;

    static void pack(const Strs &items, std::vector<uint8_t> &bytes, std::vector<uint64_t> &offs) {
        bytes.clear();
        offs.assign(1, 0);
        for (const std::string &s : items) {
            bytes.insert(bytes.end(), s.begin(), s.end());
            offs.push_back(bytes.size());
        }
        bytes.resize(bytes.size() + 1);   // never a null pointer
    }

    void put(const Strs &topics, const Vals &vals, const std::vector<uint64_t> &exp) {
        std::vector<uint8_t> bytes;
        std::vector<uint64_t> offs;
        pack(topics, bytes, offs);
        CHECK(tm_retained_put(r, topics.size(), bytes.data(), offs.data(), vals.data(), exp.data(), nullptr) == TM_OK);
        for (size_t i = 0; i < topics.size(); ++i) model[topics[i]] = Row{vals[i], exp[i]};
    }

    void del(const Strs &topics) {
        std::vector<uint8_t> bytes;
        std::vector<uint64_t> offs;
        pack(topics, bytes, offs);
        CHECK(tm_retained_delete(r, topics.size(), bytes.data(), offs.data(), nullptr) == TM_OK);
        for (const std::string &t : topics) model.erase(t);
    }

    // one call; cap < 0: n * limit
    Page page(const Strs &filters, const std::vector<uint64_t> *cursors, uint32_t limit, uint64_t scan_rows = 0, uint64_t now = 0,
              int64_t cap = -1) {
        const size_t n = filters.size();
        const uint64_t room = cap < 0 ? n * (uint64_t)limit : (uint64_t)cap;
        std::vector<uint8_t> bytes, err(n + 2, 0xEE);
        std::vector<uint64_t> offs, hit(n + 3, C64), cur(n + 2, C64);
        Vals vals(room + 4, C32);
        pack(filters, bytes, offs);
        Page p;
        p.rc = tm_retained_match_page(r, n, bytes.data(), offs.data(), now, cursors ? cursors->data() : nullptr, limit, scan_rows,
                                      hit.data() + 1, vals.data(), room, cur.data() + 1, err.data() + 1);
        CHECK(hit[0] == C64 && hit[n + 2] == C64 && cur[0] == C64 && cur[n + 1] == C64 && err[0] == 0xEE && err[n + 1] == 0xEE);
        for (uint64_t k = room; k < room + 4; ++k) CHECK(vals[k] == C32);
        CHECK(p.rc == TM_OK || p.rc == TM_ECAP);
        p.hit.assign(hit.begin() + 1, hit.begin() + n + 2);
        p.cursor.assign(cur.begin() + 1, cur.begin() + n + 1);
        p.err.assign(err.begin() + 1, err.begin() + n + 1);
        p.vals.assign(vals.begin(), vals.begin() + room);
        CHECK(p.hit[0] == 0);
        for (size_t i = 0; i < n; ++i) CHECK(p.hit[i + 1] - p.hit[i] <= limit);
        CHECK((p.rc == TM_ECAP) == (p.hit[n] > room));
        return p;
    }

    // page by page to DONE -> the values in the order they came; *calls: how many calls it took
    Vals drain(const std::string &f, uint32_t limit, uint64_t scan_rows = 0, uint64_t now = 0, uint64_t from = BEGIN,
               size_t *calls = nullptr) {
        Vals out;
        std::vector<uint64_t> cur{from};
        size_t k = 0;
        while (cur[0] != DONE) {
            const Page p = page({f}, &cur, limit, scan_rows, now);
            CHECK(p.rc == TM_OK && p.err[0] == (valid_filter(f) ? 0 : 2));
            const Vals got = p.list(0);
            if (p.cursor[0] != DONE && !scan_rows) CHECK(got.size() == limit);   // only a full page leaves a live cursor
            if (p.cursor[0] == DONE) CHECK(got.size() < limit);
            out.insert(out.end(), got.begin(), got.end());
            cur[0] = p.cursor[0];
            CHECK(++k < 100000);
        }
        if (calls) *calls = k;
        return out;
    }

    Vals want(const std::string &f, uint64_t now) const {
        Vals w;
        if (valid_filter(f))
            for (const auto &kv : model)
                if (topic_match(kv.first, f) && (kv.second.expiry == 0 || kv.second.expiry > now)) w.push_back(kv.second.value);
        std::sort(w.begin(), w.end());
        return w;
    }

    // the drain is the full match: no duplicate, the model's set; -> the sequence
    Vals check_drain(const std::string &f, uint32_t limit, uint64_t scan_rows = 0, uint64_t now = 0) {
        const Vals seq = drain(f, limit, scan_rows, now);
        Vals got = seq;
        std::sort(got.begin(), got.end());
        if (got != want(f, now)) {
            fprintf(stderr, "retain_page_check: filter '%s' limit %u: %zu values, expected %zu\n", f.c_str(), limit, got.size(),
                    want(f, now).size());
            abort();
        }
        return seq;
    }

    tm_retained_stats_t stats() {
        tm_retained_stats_t st;
        CHECK(tm_retained_stats(r, &st) == TM_OK);
        return st;
    }
};

void rows600(Strs &topics, Vals &vals, std::vector<uint64_t> &exp, uint32_t n = 600) {
    for (uint32_t i = 0; i < n; ++i) {
        topics.push_back((i % 13 == 7 ? "$m/" : "m/") + std::to_string(i % 5) + "/" + std::to_string(i));
        vals.push_back(5000 + i);
        exp.push_back(i % 4 ? 0 : 90 + i % 20);
    }
}

const Strs PAGE_FILTERS = {"#", "m/#", "m/+/+", "m/3/+", "+/+/17", "$m/#", "m/2/#", "+/4/+", "m/0/0", "m/+/599", "nope/#", "m/+",
                           "a/#/b", "m/3/#"};

// paging is the full match, and the sequence does not depend on the page size: all in the tail, all in the base,
// and 300 + 300 so that a page crosses from the base to the tail
void paging(int where) {
    World w;
    tm_retained_opts opts{64, 2000};
    CHECK(tm_retained_create(0, &opts, &w.r) == TM_OK);
    Strs topics;
    Vals vals;
    std::vector<uint64_t> exp;
    rows600(topics, vals, exp);
    const size_t first = where == 2 ? 300 : 600;
    w.put(Strs(topics.begin(), topics.begin() + first), Vals(vals.begin(), vals.begin() + first),
          std::vector<uint64_t>(exp.begin(), exp.begin() + first));
    if (where >= 1) CHECK(tm_retained_compact(w.r) == TM_OK);
    if (where == 2)
        w.put(Strs(topics.begin() + 300, topics.end()), Vals(vals.begin() + 300, vals.end()),
              std::vector<uint64_t>(exp.begin() + 300, exp.end()));
    const tm_retained_stats_t st = w.stats();
    CHECK(st.base_rows == (where == 0 ? 0u : where == 1 ? 600u : 300u) && st.base_rows + st.tail_rows == 600);
    for (const std::string &f : PAGE_FILTERS)
        for (uint64_t now : {0ull, 100ull}) {
            const Vals seq = w.check_drain(f, 1000, 0, now);
            for (uint32_t limit : {1u, 255u, 256u, 257u})
                if (limit != 1 || now == 0) CHECK(w.check_drain(f, limit, 0, now) == seq);
            CHECK(w.check_drain(f, 100, 0, now) == seq);   // every page starts mid-tile
            CHECK(w.check_drain(f, 1000, 256, now) == seq);
            CHECK(w.check_drain(f, 7, 50, now) == seq);
        }
    if (where == 0) {   // scan order is visible: an empty base returns put order
        Vals in_order;
        for (uint32_t i = 0; i < 600; ++i)
            if (i % 13 != 7) in_order.push_back(5000 + i);
        CHECK(w.drain("#", 37) == in_order);
    }
    // a cursor is the store's: taken from '#', handed to m/3/#, it clamps to that filter's range, then skips to the tail
    {
        const Vals all = w.check_drain("m/3/#", 1000);
        std::vector<uint64_t> cur{BEGIN};
        Page p = w.page({"#"}, &cur, 5);
        CHECK(p.rc == TM_OK && p.cursor[0] != DONE);
        const Vals rest = w.drain("m/3/#", 1000, 0, 0, p.cursor[0]);
        // what is left of m/3/# after the first five rows of '#' went by: a suffix of its own scan order
        CHECK(rest.size() <= all.size() && std::equal(rest.begin(), rest.end(), all.end() - rest.size()));
        if (where == 2) {
            cur[0] = (p.cursor[0] & ~((1ull << 40) - 1)) | 299;   // the last base row: past m/3/#'s range or its last row
            const Vals tail_only = w.drain("m/3/#", 1000, 0, 0, cur[0]);
            CHECK(tail_only.size() < all.size() && std::equal(tail_only.begin(), tail_only.end(), all.end() - tail_only.size()));
        }
    }
    CHECK(tm_retained_destroy(w.r) == TM_OK);
}

// n matching rows, limit = 256: the cursor after the page, the remainder, and exactly `limit` rows left
void tile_edges() {
    for (int where = 0; where < 2; ++where)
        for (uint32_t n : {255u, 256u, 257u, 512u, 513u}) {
            World w;
            tm_retained_opts opts{64, 2000};
            CHECK(tm_retained_create(0, &opts, &w.r) == TM_OK);
            Strs topics;
            Vals vals;
            for (uint32_t i = 0; i < n; ++i) {
                topics.push_back("e/" + std::to_string(1000 + i));
                vals.push_back(i);
            }
            w.put(topics, vals, std::vector<uint64_t>(n, 0));
            if (where) CHECK(tm_retained_compact(w.r) == TM_OK);
            std::vector<uint64_t> cur{BEGIN};
            Vals seen;
            for (uint32_t left = n; cur[0] != DONE;) {
                const Page p = w.page({"e/+"}, &cur, 256);
                const Vals got = p.list(0);
                CHECK(got.size() == std::min(left, 256u));
                CHECK((p.cursor[0] != DONE) == (got.size() == 256));   // exactly `limit` left: live, then ([], DONE)
                seen.insert(seen.end(), got.begin(), got.end());
                left -= (uint32_t)got.size();
                cur[0] = p.cursor[0];
            }
            CHECK(seen == vals);   // (the topics sort as they were put)
            CHECK(tm_retained_destroy(w.r) == TM_OK);
        }
    // hits in only the first wave of a tile, in only the last, and in all four
    World w;
    tm_retained_opts opts{64, 2000};
    CHECK(tm_retained_create(0, &opts, &w.r) == TM_OK);
    Strs topics;
    Vals vals;
    for (uint32_t i = 0; i < 768; ++i) {
        const uint32_t tile = i / 256, lane = i % 256;
        const bool hit = tile == 0 ? lane < 64 : tile == 1 ? lane >= 192 : lane % 3 == 0;
        topics.push_back(std::string(hit ? "h/" : "x/") + std::to_string(i));
        vals.push_back(i);
    }
    w.put(topics, vals, std::vector<uint64_t>(768, 0));
    for (uint32_t limit : {1u, 10u, 63u, 64u, 65u, 130u, 1000u}) {
        const Vals seq = w.check_drain("h/+", limit);
        CHECK(std::is_sorted(seq.begin(), seq.end()));
    }
    CHECK(tm_retained_destroy(w.r) == TM_OK);
}

// 64 filters, each at a different page of its own drain, some at DONE: every list is the same slice taken alone
void mixed_batch() {
    World w;
    tm_retained_opts opts{64, 2000};
    CHECK(tm_retained_create(0, &opts, &w.r) == TM_OK);
    Strs topics;
    Vals vals;
    std::vector<uint64_t> exp;
    rows600(topics, vals, exp);
    w.put(Strs(topics.begin(), topics.begin() + 400), Vals(vals.begin(), vals.begin() + 400),
          std::vector<uint64_t>(exp.begin(), exp.begin() + 400));
    CHECK(tm_retained_compact(w.r) == TM_OK);
    w.put(Strs(topics.begin() + 400, topics.end()), Vals(vals.begin() + 400, vals.end()),
          std::vector<uint64_t>(exp.begin() + 400, exp.end()));
    const Strs pool = {"m/0/0", "m/3/#", "m/+/17", "+/+/17", "#", "a/#/b", "m/unknown/+", "m/2/+", "+/4/+", "$m/#"};
    const uint32_t limit = 9;
    Strs filters;
    std::vector<uint64_t> cursors;
    std::vector<Vals> expect;
    std::vector<uint64_t> expect_cursor;
    for (uint32_t i = 0; i < 64; ++i) {
        const std::string f = pool[i % pool.size()];
        std::vector<uint64_t> cur{BEGIN};
        for (uint32_t k = 0; k < i / 10 && cur[0] != DONE; ++k) cur[0] = w.page({f}, &cur, limit).cursor[0];
        if (i % 17 == 16) cur[0] = DONE;
        const Page alone = w.page({f}, &cur, limit);
        filters.push_back(f);
        cursors.push_back(cur[0]);
        expect.push_back(alone.list(0));
        expect_cursor.push_back(alone.cursor[0]);
    }
    const Page p = w.page(filters, &cursors, limit);
    CHECK(p.rc == TM_OK);
    size_t some = 0, done_in = 0;
    for (uint32_t i = 0; i < 64; ++i) {
        CHECK(p.list(i) == expect[i] && p.cursor[i] == expect_cursor[i]);
        CHECK(p.err[i] == (filters[i] == "a/#/b" ? 2 : 0));
        some += !expect[i].empty();
        done_in += cursors[i] == DONE;
    }
    CHECK(some >= 25 && done_in >= 3);
    // capacity: total - 1 is TM_ECAP with the true offsets, n * limit never is
    const uint64_t total = p.hit[64];
    const Page q = w.page(filters, &cursors, limit, 0, 0, (int64_t)total - 1);
    CHECK(q.rc == TM_ECAP && q.hit == p.hit);
    const Page e = w.page(filters, &cursors, limit, 0, 0, (int64_t)total);
    CHECK(e.rc == TM_OK && e.vals == Vals(p.vals.begin(), p.vals.begin() + total));
    const Page z = w.page(filters, &cursors, limit, 0, 0, 0);
    CHECK(z.rc == TM_ECAP && z.hit == p.hit);
    CHECK(tm_retained_destroy(w.r) == TM_OK);
}

// expiry, dead rows and '$' topics
void visibility() {
    World w;
    tm_retained_opts opts{16, 6};
    CHECK(tm_retained_create(0, &opts, &w.r) == TM_OK);
    w.put({"$SYS/a", "$SYS/b/c", "t/1", "t/2", "t/3", "t/4", "u/1", "u/2", "t/5"}, {1, 2, 3, 4, 5, 6, 7, 8, 9},
          {0, 0, 0, 1000, 1001, 0, 999, 0, 0});
    w.del({"t/4", "u/2"});
    for (uint32_t limit : {1u, 2u, 100u})
        for (uint64_t now : {0ull, 999ull, 1000ull, 1001ull})
            for (const std::string &f : Strs{"#", "+/+", "$SYS/#", "t/+", "+/1", "t/4", "$SYS/+"}) w.check_drain(f, limit, 0, now);
    CHECK(w.check_drain("#", 2, 0, 1000).size() == 3 && w.check_drain("t/4", 2).empty());
    CHECK(w.check_drain("$SYS/#", 1).size() == 2 && w.check_drain("+/#", 3).size() == 5);
    CHECK(tm_retained_destroy(w.r) == TM_OK);
}

// scan_rows: 2,000 rows, +/+/leaf with 10 hits, a window of 256: short pages with live cursors to the end
void windows() {
    World w;
    tm_retained_opts opts{64, 4000};
    CHECK(tm_retained_create(0, &opts, &w.r) == TM_OK);
    Strs topics;
    Vals vals;
    for (uint32_t i = 0; i < 2000; ++i) {
        topics.push_back("s/" + std::to_string(i) + (i % 200 == 77 ? "/leaf" : "/other"));
        vals.push_back(i);
    }
    w.put(Strs(topics.begin(), topics.begin() + 1200), Vals(vals.begin(), vals.begin() + 1200), std::vector<uint64_t>(1200, 0));
    CHECK(tm_retained_compact(w.r) == TM_OK);
    w.put(Strs(topics.begin() + 1200, topics.end()), Vals(vals.begin() + 1200, vals.end()), std::vector<uint64_t>(800, 0));
    std::vector<uint64_t> cur{BEGIN};
    Vals seen;
    size_t calls = 0;
    while (cur[0] != DONE) {
        const Page p = w.page({"+/+/leaf"}, &cur, 1000, 256);
        CHECK(p.rc == TM_OK && p.list(0).size() < 1000);
        const Vals got = p.list(0);
        seen.insert(seen.end(), got.begin(), got.end());
        cur[0] = p.cursor[0];
        ++calls;
        CHECK((cur[0] != DONE) == (calls < 8));   // 7 whole windows and 208 rows: the eighth reaches the end
    }
    CHECK(calls <= (2000 + 255) / 256 + 1 && seen.size() == 10);
    std::sort(seen.begin(), seen.end());
    CHECK(seen == w.want("+/+/leaf", 0));
    // a window that ends exactly at the end of the base range, and one row short of the end of the rows
    for (uint64_t win : {1200ull, 1199ull, 1201ull, 1999ull, 2000ull, 2001ull, 1ull})
        if (win != 1) w.check_drain("+/+/leaf", 3, win); else w.check_drain("s/77/+", 1, 1);
    CHECK(tm_retained_destroy(w.r) == TM_OK);
}

// pins hold compactions back; a cursor of another epoch is stale
void pins_and_epochs() {
    World w;
    tm_retained_opts opts{16, 4};
    CHECK(tm_retained_create(0, &opts, &w.r) == TM_OK);
    CHECK(tm_retained_unpin(w.r) == TM_EINVAL && tm_retained_pin(nullptr) == TM_EINVAL && tm_retained_unpin(nullptr) == TM_EINVAL);
    Strs topics;
    Vals vals;
    for (uint32_t i = 0; i < 40; ++i) {
        topics.push_back("p/" + std::to_string(i));
        vals.push_back(i);
    }
    w.put(topics, vals, std::vector<uint64_t>(40, 0));   // past tail_max: compacted
    tm_retained_stats_t st = w.stats();
    CHECK(st.tail_rows == 0 && st.compactions == 1);
    std::vector<uint64_t> cur{BEGIN};
    Page p = w.page({"p/+"}, &cur, 7);
    Vals seen = p.list(0);
    CHECK(p.cursor[0] != DONE && tm_retained_pin(w.r) == TM_OK);
    for (uint32_t i = 0; i < 10; ++i) w.put({"q/" + std::to_string(i)}, {100 + i}, {0});
    st = w.stats();
    CHECK(st.compactions == 1 && st.tail_rows == 10);
    CHECK(tm_retained_compact(w.r) == TM_OK && w.stats().compactions == 1);   // due, not done
    const Vals rest = w.drain("p/+", 7, 0, 0, p.cursor[0]);
    seen.insert(seen.end(), rest.begin(), rest.end());
    std::sort(seen.begin(), seen.end());
    CHECK(seen == vals);   // every original row exactly once
    CHECK(w.check_drain("#", 6).size() == 50);   // rows written under the pin are in the tail
    CHECK(tm_retained_pin(w.r) == TM_OK && tm_retained_unpin(w.r) == TM_OK && w.stats().compactions == 1);
    CHECK(tm_retained_unpin(w.r) == TM_OK);
    st = w.stats();
    CHECK(st.compactions == 2 && st.tail_rows == 0 && st.base_rows == 50);
    CHECK(tm_retained_unpin(w.r) == TM_EINVAL);
    // a due compaction alone (the tail below tail_max) is done at the unpin
    CHECK(tm_retained_pin(w.r) == TM_OK && tm_retained_compact(w.r) == TM_OK && w.stats().compactions == 2);
    CHECK(tm_retained_unpin(w.r) == TM_OK && w.stats().compactions == 3);
    CHECK(tm_retained_pin(w.r) == TM_OK && tm_retained_unpin(w.r) == TM_OK && w.stats().compactions == 3);
    // stale: a live cursor without a pin, then a compaction
    cur[0] = BEGIN;
    p = w.page({"#"}, &cur, 5);
    CHECK(p.cursor[0] != DONE && p.list(0).size() == 5);
    const std::vector<uint64_t> old{p.cursor[0], BEGIN, DONE};
    CHECK(tm_retained_compact(w.r) == TM_OK);
    p = w.page({"#", "#", "#"}, &old, 5);
    CHECK(p.rc == TM_OK && p.err[0] == TM_RET_ESTALE && p.list(0).empty() && p.cursor[0] == BEGIN);
    CHECK(p.err[1] == 0 && p.list(1).size() == 5 && p.err[2] == 0 && p.list(2).empty() && p.cursor[2] == DONE);
    // null cursors are all BEGIN
    const Page q = w.page({"#", "p/+"}, nullptr, 5);
    CHECK(q.list(0) == p.list(1) && q.list(1).size() == 5);
    // the pin counter under two threads
    {
        auto work = [&] {
            for (int i = 0; i < 2000; ++i) CHECK(tm_retained_pin(w.r) == TM_OK);
            for (int i = 0; i < 2000; ++i) CHECK(tm_retained_unpin(w.r) == TM_OK);
        };
        std::thread a(work), b(work);
        a.join();
        b.join();
        CHECK(tm_retained_unpin(w.r) == TM_EINVAL);
    }
    CHECK(tm_retained_destroy(w.r) == TM_OK);
}

void arguments() {
    tm_retained *r = nullptr;
    CHECK(tm_retained_create(0, nullptr, &r) == TM_OK);
    uint64_t hit[2] = {5, 5}, offs[2] = {0, 1}, cur[1] = {7};
    uint32_t one = 0xABCD;
    const uint8_t bytes[2] = {'#', 0};
    CHECK(tm_retained_match_page(nullptr, 0, nullptr, nullptr, 0, nullptr, 1, 0, hit, nullptr, 0, cur, nullptr) == TM_EINVAL);
    CHECK(std::string(tm_retained_last_error(nullptr)).find("tm_retained_match_page") == 0);
    CHECK(tm_retained_match_page(r, 1, bytes, offs, 0, nullptr, 0, 0, hit, &one, 1, cur, nullptr) == TM_EINVAL);   // limit 0
    CHECK(tm_retained_match_page(r, 1, bytes, offs, 0, nullptr, 1, 0, nullptr, &one, 1, cur, nullptr) == TM_EINVAL);
    CHECK(tm_retained_match_page(r, 1, bytes, offs, 0, nullptr, 1, 0, hit, &one, 1, nullptr, nullptr) == TM_EINVAL);
    CHECK(tm_retained_match_page(r, 1, bytes, offs, 0, nullptr, 1, 0, hit, nullptr, 1, cur, nullptr) == TM_EINVAL);
    CHECK(tm_retained_match_page(r, 0, nullptr, nullptr, 0, nullptr, 1, 0, hit, nullptr, 0, nullptr, nullptr) == TM_OK && hit[0] == 0);
    // the empty store: nothing, DONE, no launch
    CHECK(tm_retained_match_page(r, 1, bytes, offs, 0, nullptr, 4, 0, hit, &one, 1, cur, nullptr) == TM_OK);
    CHECK(hit[1] == 0 && one == 0xABCD && cur[0] == DONE);
    tm_retained_stats_t st;
    CHECK(tm_retained_stats(r, &st) == TM_OK && st.match_launches == 0 && st.no_launch_filters == 1);
    CHECK(tm_retained_destroy(r) == TM_OK);
}

// put, delete and expire churn; after each step three random filters drained with a random limit
void seeded(uint32_t seed) {
    std::mt19937 rng(seed);
    World w;
    tm_retained_opts opts{8, 4 + seed % 5};
    CHECK(tm_retained_create(0, &opts, &w.r) == TM_OK);
    const Strs alphabet = {"a", "b", "c", "", "$s", "dd"};
    auto word = [&] { return alphabet[rng() % alphabet.size()]; };
    auto topic = [&] {
        std::string t = word();
        for (uint32_t k = rng() % (seed % 3 == 0 ? 11 : 4); k; --k) t += "/" + word();
        return t;
    };
    auto filter = [&] {
        std::string f;
        const uint32_t n = 1 + rng() % 4;
        for (uint32_t k = 0; k < n; ++k) {
            const uint32_t c = rng() % 10;
            f += (k ? "/" : "") + (c < 3 ? std::string("+") : c == 3 && k + 1 == n ? std::string("#") : word());
        }
        return f;
    };
    uint32_t v = 1;
    bool pinned = false;
    for (int step = 0; step < 200; ++step) {
        const uint32_t c = rng() % 12;
        Strs batch;
        for (uint32_t k = 1 + rng() % 3; k; --k) batch.push_back(topic());
        std::sort(batch.begin(), batch.end());
        batch.erase(std::unique(batch.begin(), batch.end()), batch.end());
        batch.erase(std::remove(batch.begin(), batch.end(), std::string()), batch.end());
        if (c < 6) {
            Vals vals;
            std::vector<uint64_t> exp;
            for (size_t k = 0; k < batch.size(); ++k) {
                vals.push_back(v++);
                exp.push_back(rng() % 3 ? 0 : 90 + rng() % 20);
            }
            w.put(batch, vals, exp);
        } else if (c < 9) {
            if (!w.model.empty() && rng() % 2) {
                auto it = w.model.begin();
                std::advance(it, rng() % w.model.size());
                batch.push_back(it->first);
            }
            w.del(batch);
        } else if (c == 9) {
            uint64_t n = 0;
            int complete = 0;
            const uint64_t deadline = 90 + rng() % 20;
            CHECK(tm_retained_expire(w.r, deadline, 0, nullptr, 0, &n, &complete) == TM_OK && complete == 1);
            for (auto it = w.model.begin(); it != w.model.end();)
                it = it->second.expiry != 0 && it->second.expiry < deadline ? w.model.erase(it) : std::next(it);
        } else if (c == 10) {
            CHECK(tm_retained_compact(w.r) == TM_OK);
        } else {
            CHECK((pinned ? tm_retained_unpin(w.r) : tm_retained_pin(w.r)) == TM_OK);
            pinned = !pinned;
        }
        const uint64_t now = rng() % 2 ? 0 : 100;
        w.check_drain(rng() % 4 ? filter() : "#", 1 + rng() % 12, rng() % 3 ? 0 : 1 + rng() % 9, now);
        for (int k = 0; k < 2; ++k) w.check_drain(filter(), 1 + rng() % 12, 0, now);
    }
    if (pinned) CHECK(tm_retained_unpin(w.r) == TM_OK);
    CHECK(w.stats().compactions >= 3);
    CHECK(tm_retained_destroy(w.r) == TM_OK);
}

}  // namespace

int main() {
    arguments();
    for (int where = 0; where < 3; ++where) paging(where);
    tile_edges();
    mixed_batch();
    visibility();
    windows();
    pins_and_epochs();
    for (uint32_t seed = 1; seed <= 6; ++seed) seeded(seed);
    CHECK(fake_hip_live_allocs() == 0);
    printf("retain page check ok\n");
    return 0;
}
