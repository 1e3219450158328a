// subs_check.cpp -- emqx_amd/csrc/tm_subs.h (the host side of tm_set_subscribers)
// on its own: seeded set / replace / clear operations against a std::map model.
// After every operation a "device copy" takes the dirty ranges (as table_upload
// does) and must equal the host arrays word for word; every few operations the
// whole structure is audited:
//   every live span lies inside the pool, no two live spans overlap, every
//   list equals the model's, values the model does not hold have count 0;
// compaction must happen, must preserve every list, and leaves a pool of at
// most 2 x the live words + one block.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>
#include <vector>

#include "../../emqx_amd/csrc/tm_subs.h"

using tmx::SubPool;

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return g_state;
}

#define CHECK(c, ...)                                  \
    do {                                               \
        if (!(c)) {                                    \
            std::fprintf(stderr, "subs_check: line %d: ", __LINE__); \
            std::fprintf(stderr, __VA_ARGS__);         \
            std::fprintf(stderr, "\n");                \
            std::exit(1);                              \
        }                                              \
    } while (0)

using Model = std::map<uint32_t, std::vector<uint32_t>>;

static uint64_t live_words(const Model &m) {
    uint64_t w = 0;
    for (const auto &kv : m) w += kv.second.size();
    return w;
}

static void audit(const SubPool &sp, const Model &m, uint64_t op) {
    CHECK(sp.span.size() % 2 == 0 && sp.cls.size() == sp.span.size() / 2, "op %llu: span / cls sizes", (unsigned long long)op);
    std::vector<std::pair<uint64_t, uint64_t>> spans;
    for (uint64_t v = 0; v < sp.values(); v++) {
        const uint64_t pos = sp.span[2 * v], cnt = sp.span[2 * v + 1];
        const auto it = m.find((uint32_t)v);
        const uint64_t want = it == m.end() ? 0 : it->second.size();
        CHECK(cnt == want, "op %llu: value %llu has %llu ids, the model %llu", (unsigned long long)op,
              (unsigned long long)v, (unsigned long long)cnt, (unsigned long long)want);
        if (!cnt) continue;
        CHECK(pos + cnt <= sp.pool.size(), "op %llu: value %llu's span ends past the pool", (unsigned long long)op,
              (unsigned long long)v);
        for (uint64_t k = 0; k < cnt; k++)
            CHECK(sp.pool[pos + k] == it->second[k], "op %llu: value %llu word %llu differs", (unsigned long long)op,
                  (unsigned long long)v, (unsigned long long)k);
        spans.emplace_back(pos, pos + cnt);
    }
    for (const auto &kv : m) CHECK(kv.second.empty() || kv.first < sp.values(), "op %llu: a value without a span", (unsigned long long)op);
    std::sort(spans.begin(), spans.end());
    for (size_t i = 1; i < spans.size(); i++)
        CHECK(spans[i - 1].second <= spans[i].first, "op %llu: two live spans overlap at %llu", (unsigned long long)op,
              (unsigned long long)spans[i].first);
    CHECK(sp.live == live_words(m), "op %llu: live is %llu, the model holds %llu", (unsigned long long)op,
          (unsigned long long)sp.live, (unsigned long long)live_words(m));
}

// the device side of table_upload: whole -> everything, else the two ranges
struct Mirror {
    std::vector<uint32_t> span, pool;
    void take(SubPool &sp, uint64_t op) {
        uint64_t slo, shi, plo, phi;
        bool whole;
        sp.take_dirty(slo, shi, plo, phi, whole);
        if (whole) {
            slo = plo = 0;
            shi = sp.span.size();
            phi = sp.pool.size();
        }
        CHECK(shi <= sp.span.size() && phi <= sp.pool.size(), "op %llu: a dirty range ends past its array", (unsigned long long)op);
        span.resize(sp.span.size(), 0xDEADBEEFu);
        pool.resize(sp.pool.size(), 0xDEADBEEFu);
        for (uint64_t i = slo; i < shi; i++) span[i] = sp.span[i];
        for (uint64_t i = plo; i < phi; i++) pool[i] = sp.pool[i];
        CHECK(span == sp.span, "op %llu: the dirty range missed a span word", (unsigned long long)op);
        CHECK(pool == sp.pool, "op %llu: the dirty range missed a pool word", (unsigned long long)op);
    }
};

int main() {
    SubPool sp;
    Model model;
    Mirror dev;
    const uint64_t OPS = 120000;
    const uint32_t VALUES = 3000;
    uint32_t next_id = 1;
    uint64_t seen = 0, long_lists = 0, in_place = 0;
    std::vector<uint32_t> ids;
    for (uint64_t op = 0; op < OPS; op++) {
        // a value past the end now and then, so the spans grow with gaps
        const uint32_t v = (rnd() % 1000 == 0) ? VALUES + (uint32_t)(rnd() % 2000) : (uint32_t)(rnd() % VALUES);
        const uint64_t kind = rnd() % 1000;
        uint32_t n;
        if (kind < 250) n = 0;                                 // clear
        else if (kind < 995) n = 1 + (uint32_t)(rnd() % 3);    // 1 .. 3
        else { n = 1000 + (uint32_t)(rnd() % 3000); long_lists++; }
        // phases of clears: the live words fall below the garbage
        if ((op / 20000) % 2 == 1 && kind < 700) n = 0;
        ids.resize(n);
        for (uint32_t k = 0; k < n; k++) ids[k] = (rnd() % 16 == 0) ? 0xFFFFFFFFu - (uint32_t)(rnd() % 3) : next_id++;
        const uint32_t old_pos = v < sp.values() ? sp.span[2 * (uint64_t)v] : 0;
        const bool had = v < sp.values() && sp.cls[v];
        const uint64_t before = sp.compactions;
        CHECK(sp.set(v, ids.data(), n), "op %llu: set refused", (unsigned long long)op);
        if (n) model[v] = ids; else model.erase(v);
        if (sp.compactions != before) {
            seen++;
            audit(sp, model, op);   // compaction preserved every list
            CHECK(sp.pool.size() <= 2 * sp.live + 4096, "op %llu: %llu pool words for %llu live ones after a compaction",
                  (unsigned long long)op, (unsigned long long)sp.pool.size(), (unsigned long long)sp.live);
            CHECK(sp.pool.size() == sp.tight, "op %llu: the compacted pool is not tight", (unsigned long long)op);
        } else if (had && n && sp.span[2 * (uint64_t)v] == old_pos) {
            in_place++;
        }
        CHECK(sp.garbage() <= sp.live, "op %llu: more garbage than lists after the call", (unsigned long long)op);
        dev.take(sp, op);
        if (op % 997 == 0 || op + 1 == OPS) audit(sp, model, op);
    }
    // a value twice: the last list stands
    const uint32_t a[3] = {7, 8, 9}, b[1] = {5};
    sp.set(42, a, 3);
    sp.set(42, b, 1);
    model[42] = {5};
    dev.take(sp, OPS);
    audit(sp, model, OPS);
    CHECK(seen >= 1 && sp.compactions == seen, "no compaction in %llu operations", (unsigned long long)OPS);
    CHECK(long_lists >= 100 && in_place >= 1000, "the history was not what it was meant to be");
    std::printf("subs ok: %llu operations, %llu compactions, %llu long lists, %llu in place, %zu pool words for %llu live\n",
                (unsigned long long)OPS, (unsigned long long)seen, (unsigned long long)long_lists,
                (unsigned long long)in_place, sp.pool.size(), (unsigned long long)sp.live);
    return 0;
}
