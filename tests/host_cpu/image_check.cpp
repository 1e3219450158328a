// image_check.cpp -- runs one scenario file of tests/image_script.py through the
// public ABI of include/tmatch.h over the CPU device fake (fake_hip.cpp,
// fake_launch.cpp), built with tm_host.cpp under -fsanitize=address,undefined
// (tests/test_image_cpu.py).
//
//   image_check <scenario file> <copies>
//   image_check --threads <operations>      (the ThreadSanitizer build's phase, below)
//
// Per step: tm_apply_deltas or tm_commit (with two copies: alternating, so a
// lagging copy takes several ring patches at once, and with a few busy events
// before each commit).  Per check step, every answer compared exactly with the
// file's expectations: tm_match_batch (staged and in place; traversal, sorted
// and unique order; once with a capacity too small), tm_first_batch,
// tm_match_batch_dev_pairs, and with small_path_ok answering true
// tm_match_batch32_ex and tm_match_batch32_pairs through the combiner
// (launch_small_segs); then the full audit of the view the last launch was
// given.  mfcheck steps: tm_matches_filter against the file's answers.  At the
// end, with two copies, a phase that makes every copy busy reaches a waited
// and a forced commit (TM_DEBUG_COMMIT_WAITS / _FORCED); the audit kinds the
// scenario claims must have non-zero counts; nothing the fake allocated may be
// left after tm_destroy.
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <unordered_set>
#include <vector>

#include "../../include/tmatch.h"
#include "fake_hip.h"
#include "image_walk.h"

using imgw::die;

namespace {

const char *CLAIMS[] = {"wide_bitmaps", "hints_both", "qq_saturated", "exact_wrapped", "ctab_wrapped", "wpool_compaction",
                        "wseq_compaction", "vocab_shrink", "exact_shrink", "node_reuse", "wid_reuse", "hdesc", "dense_both",
                        "mfilter", "wide_to_narrow", "ring_wrap", "rehash_annexed"};
constexpr int N_CLAIMS = sizeof(CLAIMS) / sizeof(CLAIMS[0]);

struct Reader {
    std::vector<uint8_t> buf;
    size_t at = 0;
    void need(size_t n) const { if (at + n > buf.size()) die("scenario file: truncated at byte %zu", at); }
    uint32_t u32() { need(4); uint32_t v; memcpy(&v, buf.data() + at, 4); at += 4; return v; }
    uint64_t u64() { need(8); uint64_t v; memcpy(&v, buf.data() + at, 8); at += 8; return v; }
    template <class T>
    std::vector<T> arr() {
        const uint64_t n = u64();
        need(n * sizeof(T));
        std::vector<T> v(n);
        if (n) memcpy(v.data(), buf.data() + at, n * sizeof(T));
        at += n * sizeof(T);
        return v;
    }
    std::string text() { auto v = arr<char>(); return std::string(v.begin(), v.end()); }
};

struct Totals {
    uint64_t checks = 0, topics = 0, api_calls = 0, audits = 0, compared = 0, audit_nodes = 0;
    uint64_t count[N_CLAIMS] = {};
    uint64_t dense_seen = 0, bitmap_seen = 0, hints0 = 0, hints1 = 0, commits = 0, applies = 0, mf_queries = 0;
    uint64_t depth_slack = 0, xlen_extra = 0, hdesc_extra = 0, bloom_extra = 0;
} T;

tm_index *H = nullptr;
int COPIES = 1;
std::string &WHAT = imgw::context();   // the step being run, for messages

#define OK(call)                                                                                         \
    do {                                                                                                 \
        const int rc_ = (call);                                                                          \
        if (rc_ != TM_OK) die("%s returned %d: %s", #call, rc_, tm_last_error(H));    \
    } while (0)

uint64_t dbg(uint32_t key) {
    uint64_t v = 0;
    OK(tm_debug_get(H, key, &v));
    return v;
}

struct Check {
    std::string label;
    std::vector<uint64_t> offs; std::vector<uint8_t> blob; std::vector<int64_t> cnt; std::vector<uint64_t> hit;
    std::vector<uint32_t> vals; std::vector<uint8_t> found; std::vector<uint32_t> first;
    uint64_t n() const { return offs.size() - 1; }
    std::string topic(uint64_t t) const { return imgw::show(blob.data() + offs[t], (size_t)std::min<uint64_t>(offs[t + 1] - offs[t], 120)); }
    uint8_t err(uint64_t t) const { return cnt[t] < 0 ? (uint8_t)-cnt[t] : 0; }
};

template <class HT>
void same_csr(const Check &c, const HT *hit, const uint32_t *vals, const uint8_t *err, const char *api, uint64_t cap = ~0ull) {
    const uint64_t n = c.n();
    for (uint64_t t = 0; t < n; t++)
        if (err[t] != c.err(t)) die("%s: err flag %u for topic '%s', the oracle says %u", api, err[t], c.topic(t).c_str(), c.err(t));
    for (uint64_t t = 0; t <= n; t++)
        if ((uint64_t)hit[t] != c.hit[t])
            die("%s: hit offset %" PRIu64 " is %" PRIu64 ", the oracle's %" PRIu64 " (topic '%s')", api, t, (uint64_t)hit[t],
                c.hit[t], c.topic(t ? t - 1 : 0).c_str());
    for (uint64_t i = 0; i < std::min<uint64_t>(c.vals.size(), cap); i++)
        if (vals[i] != c.vals[i]) {
            const uint64_t t = (uint64_t)(std::upper_bound(c.hit.begin(), c.hit.end(), i) - c.hit.begin()) - 1;
            die("%s: value %" PRIu64 " is %u, the oracle's %u (topic '%s')", api, i, vals[i], c.vals[i], c.topic(t).c_str());
        }
}

void same_pairs(const Check &c, const uint32_t *pairs, const uint32_t *vals, const uint8_t *err, const char *api) {
    const uint64_t n = c.n();
    std::vector<uint8_t> used(c.vals.size() + 1, 0);
    for (uint64_t t = 0; t < n; t++) {
        if (err[t] != c.err(t)) die("%s: err flag %u for topic '%s', the oracle says %u", api, err[t], c.topic(t).c_str(), c.err(t));
        const uint64_t want = c.hit[t + 1] - c.hit[t], pos = pairs[2 * t];
        if (pairs[2 * t + 1] != want) die("%s: %u hits for topic '%s', the oracle has %" PRIu64, api, pairs[2 * t + 1], c.topic(t).c_str(), want);
        if (pos + want > c.vals.size()) die("%s: the span of topic '%s' leaves the values", api, c.topic(t).c_str());
        for (uint64_t j = 0; j < want; j++) {
            if (used[pos + j]++) die("%s: spans overlap at %" PRIu64, api, pos + j);
            if (vals[pos + j] != c.vals[c.hit[t] + j]) die("%s: value %" PRIu64 " of topic '%s' is %u, the oracle's %u", api, j, c.topic(t).c_str(), vals[pos + j], c.vals[c.hit[t] + j]);
        }
    }
    if (pairs[2 * n] != c.vals.size()) die("%s: total %u, the oracle's %zu", api, pairs[2 * n], c.vals.size());
}

template <class X>
X *host_alloc(uint64_t count) {
    void *p = nullptr;
    OK(tm_host_alloc(H, std::max<uint64_t>(count, 1) * sizeof(X), &p));
    return static_cast<X *>(p);
}

// the audit's trackers across checks
std::unordered_map<uint32_t, uint64_t> g_node_path, g_wid_bytes;
std::unordered_map<uint32_t, uint32_t> g_word_off;
std::unordered_map<uint64_t, uint32_t> g_key_off;
uint32_t g_vmask = 0, g_xmask = 0;
std::unordered_set<uint32_t> g_wide;
bool g_anx_both = false;

void full_audit() {
    if (!fake::have_view()) die("no launch has run");
    const tmx::DevIndex ix = fake::last_view();
    imgw::AuditStats a;
    imgw::Auditor(ix, a).run();
    T.audits++;
    T.compared += a.compared;
    T.audit_nodes += a.nodes;
    T.depth_slack += a.depth_slack; T.xlen_extra += a.xlen_extra; T.hdesc_extra += a.hdesc_extra; T.bloom_extra += a.bloom_extra;
    T.count[0] += a.bitmaps;
    T.hints0 += a.hints_nonzero[0]; T.hints1 += a.hints_nonzero[1];
    T.count[1] = std::min(T.hints0, T.hints1);
    T.count[2] += a.qq_saturated;
    T.count[3] += a.exact_wrapped;
    T.count[4] += a.ctab_wrapped;
    T.count[11] += a.hdesc_nodes;
    T.dense_seen += a.dense_wide; T.bitmap_seen += a.bitmaps;
    T.count[12] = std::min(T.dense_seen, T.bitmap_seen);
    for (auto &kv : a.word_off) {   // a live long word with the same bytes at another offset: wpool was compacted
        auto f = g_word_off.find(kv.first);
        if (f != g_word_off.end() && f->second != kv.second && g_wid_bytes[kv.first] == a.wid_bytes[kv.first]) T.count[5]++;
    }
    for (auto &kv : a.key_off) {
        auto f = g_key_off.find(kv.first);
        if (f != g_key_off.end() && f->second != kv.second) T.count[6]++;
    }
    // the vocab table changed its size between two audits that both saw both annex slots held
    const bool anx_both = ix.anx_depth[0] != tmx::NONE && ix.anx_depth[1] != tmx::NONE;
    if (T.audits > 1 && ix.vmask != g_vmask && anx_both && g_anx_both) T.count[16]++;
    g_anx_both = anx_both;
    if (T.audits > 1 && ix.vmask < g_vmask) T.count[7]++;
    if (T.audits > 1 && ix.xmask < g_xmask) T.count[8]++;
    for (auto &kv : a.node_path) {   // an id on another path than before: freed and handed out again
        auto f = g_node_path.find(kv.first);
        if (f != g_node_path.end() && f->second != kv.second) T.count[9]++;
        g_node_path[kv.first] = kv.second;
    }
    for (auto &kv : a.wid_bytes) {
        auto f = g_wid_bytes.find(kv.first);
        if (f != g_wid_bytes.end() && f->second != kv.second) T.count[10]++;
        g_wid_bytes[kv.first] = kv.second;
    }
    for (uint32_t id : a.bloom_ids)   // wide at the last audit, a Bloom now: from_wide built it
        if (g_wide.count(id)) T.count[14]++;
    g_wide.clear();
    g_wide.insert(a.wide_ids.begin(), a.wide_ids.end());
    g_word_off.swap(a.word_off);
    g_key_off.swap(a.key_off);
    g_vmask = ix.vmask; g_xmask = ix.xmask;
}

void run_check(const Check &c) {
    const uint64_t n = c.n(), total = c.vals.size();
    T.checks++;
    T.topics += n;
    std::vector<uint64_t> hit(n + 1);
    std::vector<uint32_t> vals(total + 64), uq(n + 1);
    std::vector<uint8_t> err(n + 1);
    // the orders' expectations from the traversal-order answer
    std::vector<uint32_t> sorted(c.vals), uniq(c.vals), ucnt(n, 0);
    for (uint64_t t = 0; t < n; t++) {
        std::sort(sorted.begin() + c.hit[t], sorted.begin() + c.hit[t + 1]);
        std::sort(uniq.begin() + c.hit[t], uniq.begin() + c.hit[t + 1]);
        auto e = std::unique(uniq.begin() + c.hit[t], uniq.begin() + c.hit[t + 1]);
        ucnt[t] = (uint32_t)(e - (uniq.begin() + c.hit[t]));
        std::fill(e, uniq.begin() + c.hit[t + 1], 0xFFFFFFFFu);
    }
    Check cs = c, cu = c;
    cs.vals = sorted; cu.vals = uniq;

    fake::set_small_ok(false);
    // staged, traversal / sorted / unique
    OK(tm_match_batch(H, n, c.blob.data(), c.offs.data(), hit.data(), vals.data(), vals.size(), err.data()));
    same_csr(c, hit.data(), vals.data(), err.data(), "tm_match_batch");
    full_audit();
    OK(tm_match_batch_ex(H, n, c.blob.data(), c.offs.data(), hit.data(), vals.data(), vals.size(), err.data(), TM_ORDER_SORTED, nullptr));
    same_csr(cs, hit.data(), vals.data(), err.data(), "tm_match_batch_ex sorted");
    OK(tm_match_batch_ex(H, n, c.blob.data(), c.offs.data(), hit.data(), vals.data(), vals.size(), err.data(), TM_ORDER_UNIQUE, uq.data()));
    same_csr(cu, hit.data(), vals.data(), err.data(), "tm_match_batch_ex unique");
    for (uint64_t t = 0; t < n; t++)
        if (uq[t] != ucnt[t]) die("unique count %u for topic '%s', expected %u", uq[t], c.topic(t).c_str(), ucnt[t]);
    if (total >= 2) {   // a capacity too small: TM_ECAP, the offsets whole, the first cap values
        const uint64_t cap = total / 2;
        std::vector<uint32_t> part(cap);
        const int rc = tm_match_batch(H, n, c.blob.data(), c.offs.data(), hit.data(), part.data(), cap, err.data());
        if (rc != TM_ECAP) die("tm_match_batch with cap %" PRIu64 " of %" PRIu64 " returned %d, not TM_ECAP", cap, total, rc);
        same_csr(c, hit.data(), part.data(), err.data(), "tm_match_batch (TM_ECAP)", cap);
    }
    // match/2
    std::vector<uint32_t> fv(n + 1);
    std::vector<uint8_t> ff(n + 1);
    OK(tm_first_batch(H, n, c.blob.data(), c.offs.data(), fv.data(), ff.data()));
    for (uint64_t t = 0; t < n; t++)
        if (ff[t] != c.found[t] || (c.found[t] == 1 && fv[t] != c.first[t]))
            die("tm_first_batch: topic '%s': found %u value %u, the oracle's %u / %u", c.topic(t).c_str(), ff[t], fv[t], c.found[t], c.first[t]);
    // the device pairs entry (device pointers are host pointers here)
    {
        std::vector<uint32_t> pairs(2 * n + 2 + 2);
        uint32_t *pp = pairs.data() + ((reinterpret_cast<uintptr_t>(pairs.data()) & 7) ? 1 : 0);
        OK(tm_match_batch_dev_pairs(H, n, c.blob.data(), c.offs.data(), pp, vals.data(), vals.size(), err.data(), nullptr));
        same_pairs(c, pp, vals.data(), err.data(), "tm_match_batch_dev_pairs");
        if (pp[2 * n + 1] != total) die("tm_match_batch_dev_pairs: extent %u of %" PRIu64 " values", pp[2 * n + 1], total);
    }
    T.api_calls += 6;
    // in place: every buffer from tm_host_alloc
    const uint64_t nbytes = c.offs[n];
    uint8_t *pb = host_alloc<uint8_t>(nbytes + 16);
    uint64_t *po = host_alloc<uint64_t>(n + 1), *ph = host_alloc<uint64_t>(n + 1);
    uint32_t *po32 = host_alloc<uint32_t>(n + 1), *ph32 = host_alloc<uint32_t>(2 * n + 2), *pv = host_alloc<uint32_t>(total + 16);
    uint8_t *pe = host_alloc<uint8_t>(n);
    uint32_t *pf = host_alloc<uint32_t>(n);
    memcpy(pb, c.blob.data(), nbytes);
    for (uint64_t t = 0; t <= n; t++) { po[t] = c.offs[t]; po32[t] = (uint32_t)c.offs[t]; }
    const uint64_t phases0 = dbg(TM_DEBUG_PATH_PHASES), small0 = dbg(TM_DEBUG_PATH_SMALL);
    OK(tm_match_batch(H, n, pb, po, ph, pv, total + 16, pe));
    same_csr(c, ph, pv, pe, "tm_match_batch in place");
    OK(tm_first_batch(H, n, pb, po, pf, pe));
    for (uint64_t t = 0; t < n; t++)
        if (pe[t] != c.found[t] || (c.found[t] == 1 && pf[t] != c.first[t]))
            die("tm_first_batch in place: topic '%s': found %u value %u", c.topic(t).c_str(), pe[t], pf[t]);
    if (n <= 65536 && nbytes < 0xFFFFFFFFull) {
        fake::set_small_ok(true);   // the one-launch path: through the combiner to launch_small_segs
        OK(tm_match_batch32_ex(H, n, pb, po32, ph32, pv, total + 16, pe, TM_ORDER_TRAVERSAL, nullptr));
        same_csr(c, ph32, pv, pe, "tm_match_batch32_ex (one launch)");
        OK(tm_match_batch32_pairs(H, n, pb, po32, ph32, pv, total + 16, pe));
        same_pairs(c, ph32, pv, pe, "tm_match_batch32_pairs (one launch)");
        fake::set_small_ok(false);
        if (dbg(TM_DEBUG_PATH_SMALL) - small0 != 2 || dbg(TM_DEBUG_PATH_PHASES) - phases0 != 1)
            die("the in-place batches took other paths than meant (small +%" PRIu64 ", phases +%" PRIu64 ")",
                dbg(TM_DEBUG_PATH_SMALL) - small0, dbg(TM_DEBUG_PATH_PHASES) - phases0);
        T.api_calls += 2;
    }
    T.api_calls += 2;
    for (void *p : {(void *)pb, (void *)po, (void *)ph, (void *)po32, (void *)ph32, (void *)pv, (void *)pe, (void *)pf}) OK(tm_host_free(H, p));
    full_audit();
}

struct Delta { std::vector<uint8_t> ops, flags; std::vector<uint32_t> vals; std::vector<uint64_t> offs; std::vector<uint8_t> blob; };

void run_delta(const Delta &d, bool commit) {
    const uint64_t n = d.ops.size();
    if (commit) {
        if (COPIES > 1) fake_hip_busy_events(2);   // whichever lanes ask first see their batches still running
        OK(tm_commit(H, n, d.ops.data(), d.blob.data(), d.offs.data(), d.vals.data(), d.flags.data(), nullptr));
        fake_hip_busy_events(0);
        T.commits++;
    } else {
        OK(tm_apply_deltas(H, n, d.ops.data(), d.blob.data(), d.offs.data(), d.vals.data(), d.flags.data()));
        T.applies++;
    }
}

// one topic through tm_match_batch -> the replica that served it
int one_batch() {
    uint64_t before[2] = {0, 0}, after[2] = {0, 0};
    for (uint32_t r = 0; r < 2; r++) OK(tm_replica_stats(H, r, &before[r], nullptr));
    const uint8_t topic[16 + 8] = "$busy/k";
    const uint64_t offs[2] = {0, 7};
    uint64_t hit[2];
    uint32_t v[8];
    uint8_t e[1];
    OK(tm_match_batch(H, 1, topic, offs, hit, v, 8, e));
    for (uint32_t r = 0; r < 2; r++) OK(tm_replica_stats(H, r, &after[r], nullptr));
    if (after[0] - before[0] + after[1] - before[1] != 1) die("one batch, %" PRIu64 " counted", after[0] - before[0] + after[1] - before[1]);
    return after[1] != before[1];
}

// Two copies: batches left unfinished (as far as hipEventQuery tells) on both copies, then a commit.  A
// commit's own queries settle every lane, so: commit (serving copy X), a batch on X, and if X is copy 1 a
// plain delta and a batch, which runs on copy 0 (no copy is up to date, copy 0 is idle): both copies now
// hold a lane whose last batch nobody has seen finished.  With 2 busy events the next commit waits for a
// copy to drain (or, if its patch changed a view, publishes at once: forced); with events without end
// it waits out COMMIT_WAIT and is forced.
void busy_phase() {
    WHAT = "busy phase";
    const uint8_t key[] = "$busy/k";
    uint64_t offs[2] = {0, 7};
    uint32_t flip = 0;
    auto delta = [&](bool commit, uint64_t busy) {
        const uint8_t op = (flip++ & 1) ? TM_OP_DELETE : TM_OP_INSERT;
        const uint32_t val = 0xB0B0;
        fake_hip_busy_events(busy);
        if (commit) OK(tm_commit(H, 1, &op, key, offs, &val, nullptr, nullptr));
        else OK(tm_apply_deltas(H, 1, &op, key, offs, &val, nullptr));
        fake_hip_busy_events(0);
    };
    const uint8_t one = TM_OP_INSERT;
    const uint32_t v0 = 0xB0B1;
    OK(tm_apply_deltas(H, 1, &one, key, offs, &v0, nullptr));   // the key stays; its second value comes and goes
    one_batch();
    const uint64_t waits0 = dbg(TM_DEBUG_COMMIT_WAITS), forced0 = dbg(TM_DEBUG_COMMIT_FORCED);
    bool both = false;
    for (int attempt = 0; attempt < 64 && !both; attempt++) {
        delta(true, 0);
        const int x = one_batch();
        if (x != 1) continue;   // the next commit serves the other copy
        delta(false, 0);
        if (one_batch() != 0) die("busy phase: the batch after a plain delta ran on copy 1");
        const bool want_wait = dbg(TM_DEBUG_COMMIT_WAITS) == waits0;
        delta(true, want_wait ? 2 : ~0ull >> 1);
        both = dbg(TM_DEBUG_COMMIT_WAITS) > waits0 && dbg(TM_DEBUG_COMMIT_FORCED) > forced0;
    }
    if (!both)
        die("busy phase: waited commits +%" PRIu64 ", forced commits +%" PRIu64 ": both must be reached", dbg(TM_DEBUG_COMMIT_WAITS) - waits0,
            dbg(TM_DEBUG_COMMIT_FORCED) - forced0);
    if (flip & 1) delta(true, 0);
    const uint8_t del = TM_OP_DELETE;
    OK(tm_apply_deltas(H, 1, &del, key, offs, &v0, nullptr));
    one_batch();
    printf("busy phase: waited commits %" PRIu64 ", forced commits %" PRIu64 "\n", dbg(TM_DEBUG_COMMIT_WAITS), dbg(TM_DEBUG_COMMIT_FORCED));
}

// ---- threads (the ThreadSanitizer build: image_check --threads <operations>)
//
// Four threads over the fake, two copies, the busy-events knob active: one calls tm_commit, one plain
// tm_apply_deltas and tm_sync, two match -- tm_match_batch, and tm_match_batch32_pairs in place through the
// combiner with a gather window.  Each writer's delta moves ONE filter's value from epoch e - 1 to e (insert
// and delete in one delta), so whatever whole number of deltas a batch sees, each probe topic has exactly
// one value, never below the one the same reader saw before; the static filters' answers never change.

struct ThreadTopics {
    std::vector<uint8_t> blob; std::vector<uint64_t> offs; std::vector<uint32_t> offs32;
    std::vector<uint32_t> want;   // static topics: their one value
    uint64_t n() const { return offs.size() - 1; }
};

void check_answer(const ThreadTopics &tt, const char *who, const uint32_t *cnt_or_pairs, bool pairs, const uint64_t *hit,
                  const uint32_t *vals, const uint8_t *err, uint32_t last[2]) {
    for (uint64_t t = 0; t < tt.n(); t++) {
        const uint64_t c = pairs ? cnt_or_pairs[2 * t + 1] : hit[t + 1] - hit[t], pos = pairs ? cnt_or_pairs[2 * t] : hit[t];
        if (err[t] || c != 1) die("threads: %s: topic %" PRIu64 " has %" PRIu64 " hits (err %u): not a whole number of deltas", who, t, c, err[t]);
        const uint32_t v = vals[pos];
        if (t < 2) {
            if (v < last[t]) die("threads: %s: writer %" PRIu64 "'s epoch went back from %u to %u", who, t, last[t], v);
            last[t] = v;
        } else if (v != tt.want[t]) {
            die("threads: %s: static topic %" PRIu64 " gave %u, not %u", who, t, v, tt.want[t]);
        }
    }
}

int threads_main(uint64_t ops) {
    WHAT = "threads";
    COPIES = 2;
    tm_options opts{-1, 2, 0};
    OK(tm_create(&opts, &H));
    OK(tm_debug_set(H, TM_DEBUG_CMB_GATHER, 50));
    fake::set_small_ok(true);
    std::vector<std::string> keys{"ta/#", "tb/#"}, topics{"ta/x", "tb/x/y"};
    ThreadTopics tt;
    tt.want = {0, 0};
    for (int i = 0; i < 60; i++) {
        keys.push_back("s/k" + std::to_string(i) + (i % 3 ? "/+" : "/#"));
        topics.push_back("s/k" + std::to_string(i) + "/x");
        tt.want.push_back(1000 + i);
    }
    {
        std::vector<uint8_t> ops1(keys.size(), TM_OP_INSERT), blob;
        std::vector<uint64_t> offs{0};
        std::vector<uint32_t> vals{0, 0};
        for (int i = 0; i < 60; i++) vals.push_back(1000 + i);
        for (auto &k : keys) { blob.insert(blob.end(), k.begin(), k.end()); offs.push_back(blob.size()); }
        OK(tm_apply_deltas(H, keys.size(), ops1.data(), blob.data(), offs.data(), vals.data(), nullptr));
    }
    tt.offs.push_back(0);
    for (auto &t : topics) { tt.blob.insert(tt.blob.end(), t.begin(), t.end()); tt.offs.push_back(tt.blob.size()); }
    tt.blob.resize(tt.blob.size() + 16, 0);
    for (uint64_t o : tt.offs) tt.offs32.push_back((uint32_t)o);
    const uint64_t each = ops / 4, n = tt.n();
    auto writer = [&](int w) {
        const std::string key = w ? "tb/#" : "ta/#";
        const uint8_t op[2] = {TM_OP_INSERT, TM_OP_DELETE};
        std::vector<uint8_t> blob(key.begin(), key.end());
        blob.insert(blob.end(), key.begin(), key.end());
        const uint64_t offs[3] = {0, key.size(), 2 * key.size()};
        for (uint64_t e = 1; e <= each; e++) {
            const uint32_t vals[2] = {(uint32_t)e, (uint32_t)(e - 1)};
            if (e % 7 == 0) fake_hip_busy_events(3);
            int rc = w ? tm_apply_deltas(H, 2, op, blob.data(), offs, vals, nullptr) : tm_commit(H, 2, op, blob.data(), offs, vals, nullptr, nullptr);
            if (rc == TM_OK && w) rc = tm_sync(H, nullptr);
            if (rc != TM_OK) die("threads: writer %d: rc %d: %s", w, rc, tm_last_error(H));
        }
    };
    auto reader = [&](int in_place) {
        uint32_t last[2] = {0, 0};
        std::vector<uint64_t> hit(n + 1);
        std::vector<uint32_t> vals(4 * n);
        std::vector<uint8_t> err(n);
        uint8_t *pb = nullptr, *pe = nullptr;
        uint32_t *po = nullptr, *pp = nullptr, *pv = nullptr;
        if (in_place) {
            pb = host_alloc<uint8_t>(tt.blob.size()); po = host_alloc<uint32_t>(n + 1); pp = host_alloc<uint32_t>(2 * n + 2);
            pv = host_alloc<uint32_t>(4 * n); pe = host_alloc<uint8_t>(n);
            memcpy(pb, tt.blob.data(), tt.blob.size());
            memcpy(po, tt.offs32.data(), 4 * (n + 1));
        }
        for (uint64_t i = 0; i < each; i++) {
            if (in_place) {
                const int rc = tm_match_batch32_pairs(H, n, pb, po, pp, pv, 4 * n, pe);
                if (rc != TM_OK) die("threads: tm_match_batch32_pairs: rc %d: %s", rc, tm_last_error(H));
                check_answer(tt, "tm_match_batch32_pairs", pp, true, nullptr, pv, pe, last);
            } else {
                const int rc = tm_match_batch(H, n, tt.blob.data(), tt.offs.data(), hit.data(), vals.data(), vals.size(), err.data());
                if (rc != TM_OK) die("threads: tm_match_batch: rc %d: %s", rc, tm_last_error(H));
                check_answer(tt, "tm_match_batch", nullptr, false, hit.data(), vals.data(), err.data(), last);
            }
        }
        if (last[0] > each || last[1] > each) die("threads: an epoch past the writers' last");
    };
    std::thread a(writer, 0), b(writer, 1), c(reader, 0), d(reader, 1);
    a.join(); b.join(); c.join(); d.join();
    fake_hip_busy_events(0);
    uint32_t last[2] = {(uint32_t)each, (uint32_t)each};   // both writers done: the final answer
    std::vector<uint64_t> hit(n + 1);
    std::vector<uint32_t> vals(4 * n);
    std::vector<uint8_t> err(n);
    OK(tm_match_batch(H, n, tt.blob.data(), tt.offs.data(), hit.data(), vals.data(), vals.size(), err.data()));
    check_answer(tt, "the final batch", nullptr, false, hit.data(), vals.data(), err.data(), last);
    full_audit();
    const fake::Counts fc = fake::counts();
    printf("threads: %" PRIu64 " operations; commits %" PRIu64 " (waited %" PRIu64 ", forced %" PRIu64 "), combined launches %" PRIu64
           " carrying %" PRIu64 " batches, patch launches %" PRIu64 "\n", 4 * each, dbg(TM_DEBUG_COMMITS), dbg(TM_DEBUG_COMMIT_WAITS),
           dbg(TM_DEBUG_COMMIT_FORCED), dbg(TM_DEBUG_COMBINED_LAUNCHES), dbg(TM_DEBUG_COMBINED_BATCHES), fc.patch);
    if (fc.unsupported) die("threads: a launcher the fake does not implement was reached");
    OK(tm_destroy(H));
    if (fake_hip_live_allocs()) die("%zu device or pinned allocations left after tm_destroy", fake_hip_live_allocs());
    printf("image check ok\n");
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 3 && !strcmp(argv[1], "--threads")) return threads_main(strtoull(argv[2], nullptr, 10));
    if (argc != 3) { fprintf(stderr, "usage: image_check <scenario file> <copies> | --threads <operations>\n"); return 2; }
    COPIES = atoi(argv[2]);
    Reader rd;
    {
        FILE *f = fopen(argv[1], "rb");
        if (!f) die("cannot open %s", argv[1]);
        fseek(f, 0, SEEK_END);
        const long sz = ftell(f);
        fseek(f, 0, SEEK_SET);
        rd.buf.resize((size_t)sz);
        if (sz && fread(rd.buf.data(), 1, (size_t)sz, f) != (size_t)sz) die("cannot read %s", argv[1]);
        fclose(f);
    }
    rd.need(4);
    if (memcmp(rd.buf.data(), "TMIS", 4)) die("%s is no scenario file", argv[1]);
    rd.at = 4;
    if (rd.u32() != 2) die("scenario file version");
    const uint32_t claims = rd.u32(), patch_ring = rd.u32();
    const std::string name = rd.text();
    tm_options opts{-1, (uint32_t)COPIES, 0};
    WHAT = "tm_create";
    OK(tm_create(&opts, &H));
    uint64_t step = 0, deltas = 0;
    const Check *last = nullptr;
    Check cur;
    for (;;) {
        const uint32_t kind = rd.u32();
        if (!kind) break;
        step++;
        if (kind == 1 || kind == 2) {
            Delta d;
            d.ops = rd.arr<uint8_t>(); d.flags = rd.arr<uint8_t>(); d.vals = rd.arr<uint32_t>(); d.offs = rd.arr<uint64_t>();
            d.blob = rd.arr<uint8_t>();
            WHAT = name + " step " + std::to_string(step) + " (delta of " + std::to_string(d.ops.size()) + ")";
            run_delta(d, COPIES > 1 ? (deltas & 1) == 0 : kind == 2);
            deltas++;
        } else if (kind == 3) {
            cur.label = rd.text();
            cur.offs = rd.arr<uint64_t>(); cur.blob = rd.arr<uint8_t>(); cur.cnt = rd.arr<int64_t>(); cur.hit = rd.arr<uint64_t>();
            cur.vals = rd.arr<uint32_t>(); cur.found = rd.arr<uint8_t>(); cur.first = rd.arr<uint32_t>();
            WHAT = name + " step " + std::to_string(step) + " (check: " + cur.label + ", copies " + std::to_string(COPIES) + ")";
            run_check(cur);
            last = &cur;
        } else if (kind == 4) {
            const std::string label = rd.text();
            auto offs = rd.arr<uint64_t>();
            auto blob = rd.arr<uint8_t>();
            auto hit = rd.arr<uint64_t>();
            auto vals = rd.arr<uint32_t>();
            WHAT = name + " step " + std::to_string(step) + " (matches_filter: " + label + ")";
            const uint64_t n = offs.size() - 1;
            std::vector<uint64_t> gh(n + 1);
            std::vector<uint32_t> gv(vals.size() + 16);
            std::vector<uint8_t> ge(n + 1);
            OK(tm_matches_filter(H, n, blob.data(), offs.data(), gh.data(), gv.data(), gv.size(), ge.data()));
            for (uint64_t q = 0; q < n; q++) {
                const std::string flt = imgw::show(blob.data() + offs[q], (size_t)(offs[q + 1] - offs[q]));
                if (ge[q]) die("err %u for filter '%s'", ge[q], flt.c_str());
                if (gh[q + 1] != hit[q + 1]) die("filter '%s': offset %" PRIu64 ", the oracle's %" PRIu64, flt.c_str(), gh[q + 1], hit[q + 1]);
                for (uint64_t i = hit[q]; i < hit[q + 1]; i++)
                    if (gv[i] != vals[i]) die("filter '%s': value %" PRIu64 " is %u, the oracle's %u", flt.c_str(), i - hit[q], gv[i], vals[i]);
            }
            T.mf_queries += n;
            T.count[13] += n;
        } else {
            die("scenario file: step kind %u", kind);
        }
    }
    if (COPIES > 1) {
        busy_phase();
        if (last) {
            WHAT = name + " (the last check again, after the busy phase)";
            run_check(*last);
        }
    }
    const imgw::UseStats u = fake::use_stats();
    const fake::Counts fc = fake::counts();
    printf("scenario %s copies %d: %" PRIu64 " steps, %" PRIu64 " plain deltas, %" PRIu64 " commits, %" PRIu64 " checks, %" PRIu64
           " probe topics, %" PRIu64 " filter queries\n", name.c_str(), COPIES, step, T.applies, T.commits, T.checks, T.topics, T.mf_queries);
    printf("  walker: %" PRIu64 " topics walked, %" PRIu64 " nodes visited, %" PRIu64 " hits; audit by use: psum %" PRIu64 ", slot sums %" PRIu64
           ", Bloom bits %" PRIu64 ", bitmap bits %" PRIu64 ", hints %" PRIu64 " / %" PRIu64 ", fingerprints %" PRIu64 " (+%" PRIu64
           " path slots); seeks %" PRIu64 ", cuts %" PRIu64 "\n", u.topics, u.nodes, u.hits, u.psum_used, u.slot_sum_used, u.bloom_used, u.wbits_used,
           u.hint_used[0], u.hint_used[1], u.xfp_used, u.xfp_path_slots, u.seeks, u.cuts);
    printf("  full audit: %" PRIu64 " runs, %" PRIu64 " nodes, %" PRIu64 " derived words compared; slack reported: depth %" PRIu64
           ", key lengths %" PRIu64 ", hdesc %" PRIu64 ", stale Bloom bits %" PRIu64 "\n", T.audits, T.audit_nodes, T.compared, T.depth_slack, T.xlen_extra,
           T.hdesc_extra, T.bloom_extra);
    printf("  fake: match %" PRIu64 ", pairs %" PRIu64 ", first %" PRIu64 ", small_segs %" PRIu64 ", patch launches %" PRIu64 " (%" PRIu64
           " runs), matches_filter %" PRIu64 ", sort %" PRIu64 ", unsupported %" PRIu64 "\n", fc.match, fc.pairs, fc.first, fc.small_segs, fc.patch,
           fc.patch_runs, fc.mfilter, fc.sort, fc.unsupported);
    // two copies: more patches than the ring has slots went to each copy (every patch is launched once per copy)
    T.count[15] = COPIES > 1 && fc.patch > 2ull * patch_ring && T.commits > patch_ring ? fc.patch : 0;
    if (COPIES == 1) T.count[15] = 1;   // (one copy: nothing lags, the claim is the two-copy run's)
    printf("  kinds:");
    for (int i = 0; i < N_CLAIMS; i++) printf(" %s=%" PRIu64 "%s", CLAIMS[i], T.count[i], (claims >> i) & 1 ? "*" : "");
    printf("\n");
    if (fc.unsupported) die("%s: %" PRIu64 " calls reached a launcher the fake does not implement", name.c_str(), fc.unsupported);
    for (int i = 0; i < N_CLAIMS; i++)
        if (((claims >> i) & 1) && !T.count[i]) die("%s claims to exercise %s, the count is zero", name.c_str(), CLAIMS[i]);
    if (COPIES > 1 && T.commits > (uint64_t)tmx::N_TABLES && fc.patch == 0) die("%s: no patch was ever launched", name.c_str());
    WHAT = "tm_destroy";
    OK(tm_destroy(H));
    if (fake_hip_live_allocs()) die("%zu device or pinned allocations left after tm_destroy", fake_hip_live_allocs());
    printf("image check ok\n");
    return 0;
}
