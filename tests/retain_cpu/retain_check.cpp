// retain_check.cpp -- the retained store's host side (emqx_amd/csrc/tm_retain_host.cpp)
// on the CPU device fake, driven through the public ABI (tests/test_retain_image_cpu.py).
//
// A model (topic -> value, expiry) and a restatement of emqx_topic:match/2 over
// strings give every expected list; fake_retain_launch.cpp audits the image and
// the segments on every match.  Built with -fsanitize=address,undefined.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "../../include/tmatch.h"

extern "C" size_t fake_hip_live_allocs(void);

namespace {

#define CHECK(x)                                                        \
    do {                                                                \
        if (!(x)) {                                                     \
            fprintf(stderr, "retain_check: %s:%d: %s\n", __FILE__, __LINE__, #x); \
            abort();                                                    \
        }                                                               \
    } while (0)

using Strs = std::vector<std::string>;

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

struct World {
    tm_retained *r = nullptr;
    std::map<std::string, Row> model;

    void pack(const Strs &items, std::vector<uint8_t> &bytes, std::vector<uint64_t> &offs) {
        bytes.clear();
        offs.assign(1, 0);
        for (const std::string &s : items) {
            bytes.insert(bytes.end(), s.begin(), s.end());
            offs.push_back(bytes.size());
        }
        bytes.resize(bytes.size() + 1);   // never a null pointer
    }

    std::vector<uint8_t> put(const Strs &topics, const std::vector<uint32_t> &vals, const std::vector<uint64_t> &exp) {
        std::vector<uint8_t> bytes, code(topics.size(), 9);
        std::vector<uint64_t> offs;
        pack(topics, bytes, offs);
        CHECK(tm_retained_put(r, topics.size(), bytes.data(), offs.data(), vals.data(), exp.data(), code.data()) == TM_OK);
        for (size_t i = 0; i < topics.size(); ++i) {
            bool valid = !topics[i].empty();
            for (const std::string &w : split(topics[i])) valid = valid && w != "+" && w != "#";
            CHECK(code[i] == (!valid ? 2 : model.count(topics[i]) ? 0 : 1));
            if (valid) model[topics[i]] = Row{vals[i], exp[i]};
        }
        return code;
    }

    void del(const Strs &topics) {
        std::vector<uint8_t> bytes, found(topics.size(), 9);
        std::vector<uint64_t> offs;
        pack(topics, bytes, offs);
        CHECK(tm_retained_delete(r, topics.size(), bytes.data(), offs.data(), found.data()) == TM_OK);
        for (size_t i = 0; i < topics.size(); ++i) CHECK(found[i] == model.erase(topics[i]));
    }

    // every filter's list against the model, as sorted multisets (a duplicate would show)
    void match(const Strs &filters, uint64_t now) {
        std::vector<uint8_t> bytes, err(filters.size(), 9);
        std::vector<uint64_t> offs, hit(filters.size() + 1, 77);
        pack(filters, bytes, offs);
        int rc = tm_retained_match(r, filters.size(), bytes.data(), offs.data(), now, hit.data(), nullptr, 0, err.data());
        const uint64_t total = hit[filters.size()];
        CHECK(rc == (total ? TM_ECAP : TM_OK));
        std::vector<uint32_t> vals(total + 1, 0xDEADBEEF);
        CHECK(tm_retained_match(r, filters.size(), bytes.data(), offs.data(), now, hit.data(), vals.data(), total, err.data()) == TM_OK);
        CHECK(vals[total] == 0xDEADBEEF && hit[0] == 0 && hit[filters.size()] == total);
        for (size_t i = 0; i < filters.size(); ++i) {
            std::vector<uint32_t> want, got(vals.begin() + hit[i], vals.begin() + hit[i + 1]);
            const bool valid = valid_filter(filters[i]);
            CHECK(err[i] == (valid ? 0 : 2));
            if (valid)
                for (const auto &kv : model)
                    if (topic_match(kv.first, filters[i]) && (kv.second.expiry == 0 || kv.second.expiry > now))
                        want.push_back(kv.second.value);
            std::sort(want.begin(), want.end());
            std::sort(got.begin(), got.end());
            if (want != got) {
                fprintf(stderr, "retain_check: filter '%s': %zu values, expected %zu\n", filters[i].c_str(), got.size(), want.size());
                abort();
            }
        }
    }

    tm_retained_stats_t stats() {
        tm_retained_stats_t st;
        CHECK(tm_retained_stats(r, &st) == TM_OK);
        CHECK(st.live_rows == model.size() && st.base_rows + st.tail_rows == st.live_rows + st.dead_rows);
        return st;
    }
};

const Strs FILTERS = {"#", "+", "+/+", "a/#", "a/+", "a/b", "a/b/#", "+/b/#", "a/+/c", "$SYS/#", "$SYS/+", "+/#", "/+", "/#",
                      "a//b", "a/+/b", "a/", "nope/#", "a/nope", "a/#/b", "", "x/y/+/+", "b/+/+/d/#",
                      "l1/l2/l3/l4/l5/l6/l7/l8", "l1/l2/l3/l4/l5/l6/l7/l8/#", "l1/l2/l3/l4/l5/l6/l7/l8/l9",
                      "l1/l2/l3/l4/l5/l6/l7/+/l9", "l1/l2/l3/l4/l5/l6/l7/l8/+", "l1/+/l3/l4/l5/l6/l7/l8/l9/l10/l11/l12",
                      "l1/l2/l3/l4/l5/l6/l7/l8/l9/#", "l1/l2/l3/l4/l5/l6/l7/l8/l9/+/l11/#", "+/l2/l3/l4/l5/l6/l7/l8/x9"};

void scripted() {
    World w;
    tm_retained_opts opts{4, 4};
    CHECK(tm_retained_create(0, &opts, &w.r) == TM_OK);
    w.match(FILTERS, 0);                                     // the empty store
    const uint64_t words0 = w.stats().words;
    // growth across initial_rows and compactions at tail_max = 4, one topic a batch
    const Strs topics = {"a", "a/b", "a/b/c", "a/", "a//b", "/x", "$SYS/up", "$SYS/a/b", "b", "b/q/r/d", "b/q/r/d/e", "x/y/z/w",
                         "l1/l2/l3/l4/l5/l6/l7", "l1/l2/l3/l4/l5/l6/l7/l8", "l1/l2/l3/l4/l5/l6/l7/l8/l9",
                         "l1/l2/l3/l4/l5/l6/l7/x8/l9", "l1/l2/l3/l4/l5/l6/l7/l8/x9",
                         "l1/l2/l3/l4/l5/l6/l7/l8/l9/l10/l11/l12", "l1/l2/l3/l4/l5/l6/l7/l8/l9/l10/x11/l12", "a/+", "", "#/a"};
    uint32_t v = 100;
    for (const std::string &t : topics) {
        w.put({t}, {v++}, {0});
        w.match(FILTERS, 0);
    }
    tm_retained_stats_t st = w.stats();
    CHECK(st.growths >= 2 && st.compactions >= 3 && st.rt_cols == 8 && st.rt_tile == 256);
    // replace in place, base and tail, with expiries around now = 1000: > for match, >= for get
    CHECK(tm_retained_compact(w.r) == TM_OK);
    w.put({"t/new", "t/new2"}, {1, 2}, {0, 0});              // two tail rows
    w.put({"a", "a/b", "t/new", "t/new2", "a/b/c"}, {7, 8, 9, 10, 11}, {999, 1000, 1001, 1000, 0});
    for (uint64_t now : {0ull, 999ull, 1000ull, 1001ull, 1002ull}) w.match(FILTERS, now);
    w.match({"a", "a/b", "t/new", "t/+", "t/new2"}, 1000);
    {
        std::vector<uint8_t> bytes, found(4);
        std::vector<uint64_t> offs;
        std::vector<uint32_t> val(4);
        w.pack({"a", "a/b", "t/new", "none"}, bytes, offs);
        CHECK(tm_retained_get(w.r, 4, bytes.data(), offs.data(), 1000, val.data(), found.data()) == TM_OK);
        CHECK(!found[0] && found[1] && val[1] == 8 && found[2] && val[2] == 9 && !found[3]);   // expiry == now: get sees it
    }
    // delete then put again, in the base and in the tail, before and after a compaction
    w.del({"a/b", "t/new", "never/stored", "a/b"});
    w.match(FILTERS, 0);
    w.match({"t/#", "a/b"}, 0);
    w.put({"a/b", "t/new"}, {21, 22}, {0, 0});
    w.match({"t/#", "a/b", "a/#"}, 0);
    w.del({"a/b", "t/new"});
    CHECK(tm_retained_compact(w.r) == TM_OK);
    w.match({"t/#", "a/b", "a/#"}, 0);
    w.put({"a/b", "t/new"}, {31, 32}, {0, 0});
    w.match(FILTERS, 0);
    w.match({"t/#", "a/b", "a/#"}, 0);
    // clear_expired: limit, then all
    {
        uint32_t out[8];
        uint64_t n = 0;
        int complete = -1;
        w.put({"e/1", "e/2", "e/3", "e/keep"}, {41, 42, 43, 44}, {10, 20, 30, 5000});
        CHECK(tm_retained_expire(w.r, 100, 2, out, 8, &n, &complete) == TM_OK && n == 2 && complete == 0);
        for (uint64_t i = 0; i < n; ++i)
            for (auto it = w.model.begin(); it != w.model.end(); ++it)
                if (it->second.value == out[i]) {
                    CHECK(it->second.expiry != 0 && it->second.expiry < 100);
                    w.model.erase(it);
                    break;
                }
        w.match({"e/#"}, 0);
        CHECK(tm_retained_expire(w.r, 100, 0, out, 8, &n, &complete) == TM_OK && n == 1 && complete == 1);
        for (auto it = w.model.begin(); it != w.model.end();)
            it = it->second.expiry != 0 && it->second.expiry < 100 ? w.model.erase(it) : std::next(it);
        w.match({"e/#", "#"}, 0);
        CHECK(tm_retained_expire(w.r, 100, 0, nullptr, 0, &n, &complete) == TM_OK && n == 0 && complete == 1);
    }
    // dictionary ids are freed at compaction and reused: 3 * tail_max distinct words come and go
    CHECK(tm_retained_compact(w.r) == TM_OK);
    const uint64_t words1 = w.stats().words;
    Strs fresh;
    for (int i = 0; i < 12; ++i) fresh.push_back("a/fresh" + std::to_string(i));
    for (const std::string &t : fresh) w.put({t}, {v++}, {0});
    CHECK(w.stats().words == words1 + 12);
    w.match({"a/+", "a/fresh3"}, 0);
    w.del(fresh);
    CHECK(tm_retained_compact(w.r) == TM_OK);
    CHECK(w.stats().words == words1);
    for (int i = 0; i < 12; ++i) w.put({"a/again" + std::to_string(i)}, {v++}, {0});   // the freed ids again
    w.match(FILTERS, 0);
    w.match({"a/+", "a/again3", "a/fresh3"}, 0);
    // everything deleted: the dictionary is back where it began
    Strs all;
    for (const auto &kv : w.model) all.push_back(kv.first);
    w.del(all);
    CHECK(tm_retained_compact(w.r) == TM_OK);
    st = w.stats();
    CHECK(st.words == words0 && st.live_rows == 0 && st.base_rows == 0 && st.tail_rows == 0);
    w.match(FILTERS, 0);
    tm_retained_destroy(w.r);
}

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
    for (int step = 0; step < 300; ++step) {
        const uint32_t c = rng() % 10;
        Strs batch;
        for (uint32_t k = 1 + rng() % 3; k; --k) batch.push_back(topic());
        std::sort(batch.begin(), batch.end());
        batch.erase(std::unique(batch.begin(), batch.end()), batch.end());
        batch.erase(std::remove(batch.begin(), batch.end(), std::string()), batch.end());
        if (c < 6) {
            std::vector<uint32_t> vals;
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
        } else {
            CHECK(tm_retained_compact(w.r) == TM_OK);
        }
        Strs fs;
        for (int k = 0; k < 6; ++k) fs.push_back(filter());
        w.match(fs, rng() % 2 ? 0 : 100);
        w.stats();
    }
    w.match(FILTERS, 100);
    const tm_retained_stats_t st = w.stats();
    CHECK(st.compactions >= 3 && st.growths >= 1);
    tm_retained_destroy(w.r);
}

// segments of several tiles, in the base and in the tail: a filter's tiles straddle launches when the host side is
// built with a small RT_LAUNCH_TILES
void wide() {
    World w;
    tm_retained_opts opts{64, 2000};
    CHECK(tm_retained_create(0, &opts, &w.r) == TM_OK);
    Strs topics;
    std::vector<uint32_t> vals;
    std::vector<uint64_t> exp;
    for (uint32_t i = 0; i < 900; ++i) {
        topics.push_back((i % 13 == 7 ? "$m/" : "m/") + std::to_string(i % 5) + "/" + std::to_string(i));
        vals.push_back(5000 + i);
        exp.push_back(i % 4 ? 0 : 90 + i % 20);
    }
    w.put(Strs(topics.begin(), topics.begin() + 600), {vals.begin(), vals.begin() + 600}, {exp.begin(), exp.begin() + 600});
    CHECK(tm_retained_compact(w.r) == TM_OK);
    w.put(Strs(topics.begin() + 600, topics.end()), {vals.begin() + 600, vals.end()}, {exp.begin() + 600, exp.end()});
    const tm_retained_stats_t st = w.stats();
    CHECK(st.base_rows == 600 && st.tail_rows == 300);
    const Strs fs = {"#", "m/+/+", "m/3/+", "+/+/17", "m/#", "$m/#", "m/2/#", "+/4/+", "m/0/0", "m/+/299", "m/+/899", "nope/#", "m/+"};
    for (uint64_t now : {0ull, 100ull}) w.match(fs, now);
    CHECK(tm_retained_destroy(w.r) == TM_OK);
}

void arguments() {
    tm_retained *r = nullptr;
    CHECK(tm_retained_create(0, nullptr, nullptr) == TM_EINVAL);
    CHECK(tm_retained_put(nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == TM_EINVAL);
    CHECK(std::string(tm_retained_last_error(nullptr)).find("tm_retained_put") == 0);
    CHECK(tm_retained_create(0, nullptr, &r) == TM_OK);
    uint64_t hit[2] = {5, 5}, offs[2] = {0, 1};
    uint32_t one = 0xABCD;
    const uint8_t bytes[2] = {'#', 0};
    CHECK(tm_retained_match(r, 1, bytes, offs, 0, nullptr, nullptr, 0, nullptr) == TM_EINVAL);
    CHECK(tm_retained_match(r, 1, bytes, offs, 0, hit, nullptr, 4, nullptr) == TM_EINVAL);
    CHECK(tm_retained_match(r, 0, nullptr, nullptr, 0, hit, nullptr, 0, nullptr) == TM_OK && hit[0] == 0);
    CHECK(tm_retained_match(r, 1, bytes, offs, 0, hit, &one, 1, nullptr) == TM_OK && hit[1] == 0 && one == 0xABCD);
    tm_retained_stats_t st;
    CHECK(tm_retained_stats(r, &st) == TM_OK && st.match_launches == 0 && st.no_launch_filters == 1);
    CHECK(tm_retained_destroy(r) == TM_OK);
    CHECK(tm_retained_destroy(nullptr) == TM_EINVAL);
}

}  // namespace

int main() {
    arguments();
    scripted();
    wide();
    for (uint32_t seed = 1; seed <= 6; ++seed) seeded(seed);
    CHECK(fake_hip_live_allocs() == 0);
    printf("retain check ok\n");
    return 0;
}
