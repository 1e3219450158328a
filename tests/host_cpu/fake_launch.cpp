// fake_launch.cpp -- the 28 tmx:: symbols tm_host.cpp links against, on the CPU
// (tests/test_image_cpu.py).
//
// launch_match, launch_match_pairs, launch_first and launch_small_segs run the
// reference walker of image_walk.h over the view they are given and write what
// the kernels write: CSR offsets with the total in hit_offs[n], the err flags 1
// and 2, the values cut at `cap`, pairs with the total (and the extent) behind
// them, the first value with its found code.  launch_patch is k_patch's
// definition, with every run checked against the size of the table it patches.
// launch_matches_filter is the ordered filter walk, one query after another.
// launch_sort_segments and launch_copy_values are here because tm_match_batch
// in TM_ORDER_SORTED / TM_ORDER_UNIQUE cannot avoid them.  Every other launcher
// answers hipErrorNotSupported: the driver calls nothing that reaches one.
//
// small_path_ok answers what the driver last set (fake::set_small_ok) for a
// batch of 1 .. 65536 topics: true sends tm_match_batch32_ex / _pairs through
// the combiner to launch_small_segs, false sends every batch to launch_match /
// launch_first.  fanout_two_pass keeps its definition.
#include <algorithm>
#include <atomic>
#include <mutex>
#include <vector>

#include "fake_hip.h"
#include "image_walk.h"

namespace {

std::mutex g_mu;
tmx::DevIndex g_view;
bool g_have_view = false;
std::atomic<bool> g_small_ok{false};
fake::Counts g_counts{};
imgw::UseStats g_use;

void note_view(const tmx::DevIndex &ix) {
    std::lock_guard<std::mutex> g(g_mu);
    g_view = ix;
    g_have_view = true;
}

template <class OT>
struct TopicSrc {
    const uint8_t *bytes; const OT *offs;
    const uint8_t *ptr(uint64_t t) const { return bytes + offs[t]; }
    uint32_t len(uint64_t t) const { return (uint32_t)(offs[t + 1] - offs[t]); }
};

// one batch as a CSR (hit: n + 1 offsets) or as pairs (hit: 2 n + 1 words, u32)
template <class OT, class HT>
void run_batch(const tmx::DevIndex &ix, uint64_t n, const uint8_t *bytes, const OT *offs, HT *hit, bool pairs, uint8_t *err,
               uint32_t *out, uint64_t cap, bool extent) {
    imgw::UseStats st;
    imgw::Walker w(ix, st);
    TopicSrc<OT> src{bytes, offs};
    std::vector<uint32_t> vals;
    uint64_t pos = 0;
    auto sat = [](uint64_t v) { return (HT)(sizeof(HT) == 4 && v > 0xFFFFFFFFull ? 0xFFFFFFFFull : v); };
    for (uint64_t t = 0; t < n; t++) {
        vals.clear();
        const int e = w.match(src.ptr(t), src.len(t), vals);
        if (err) err[t] = (uint8_t)e;
        if (pairs) { hit[2 * t] = sat(pos); hit[2 * t + 1] = sat(vals.size()); }
        else hit[t] = sat(pos);
        for (uint32_t v : vals) { if (pos < cap && out) out[pos] = v; pos++; }
    }
    if (pairs) { hit[2 * n] = sat(pos); if (extent) hit[2 * n + 1] = sat(pos); }
    else hit[n] = sat(pos);
    std::lock_guard<std::mutex> g(g_mu);
    g_use.topics += st.topics; g_use.nodes += st.nodes; g_use.hits += st.hits; g_use.cuts += st.cuts; g_use.seeks += st.seeks;
    g_use.psum_used += st.psum_used; g_use.slot_sum_used += st.slot_sum_used; g_use.bloom_used += st.bloom_used;
    g_use.wbits_used += st.wbits_used; g_use.hint_used[0] += st.hint_used[0]; g_use.hint_used[1] += st.hint_used[1];
    g_use.xfp_used += st.xfp_used; g_use.xfp_path_slots += st.xfp_path_slots;
}

hipError_t unsupported() {
    std::lock_guard<std::mutex> g(g_mu);
    g_counts.unsupported++;
    return hipErrorNotSupported;
}

}  // namespace

namespace fake {
const tmx::DevIndex &last_view() { return g_view; }
bool have_view() { return g_have_view; }
void set_small_ok(bool on) { g_small_ok.store(on); }
Counts counts() { std::lock_guard<std::mutex> g(g_mu); return g_counts; }
imgw::UseStats use_stats() { std::lock_guard<std::mutex> g(g_mu); return g_use; }
}  // namespace fake

namespace tmx {

bool small_path_ok(const DevIndex &, uint64_t n) { return n && n <= 65536 && g_small_ok.load(); }
bool fanout_two_pass(uint32_t n_dests) { return n_dests + 1 > 256; }

hipError_t launch_match(const DevIndex &ix, const Workspace &, uint64_t n, const uint8_t *bytes, const uint64_t *offs,
                        uint64_t *hit_offs, uint8_t *err, uint32_t *out, uint64_t cap, uint32_t, LbCtl, bool phases, int,
                        hipStream_t, hipEvent_t, hipEvent_t, int *path) {
    note_view(ix);
    if (path) *path = n && !phases && small_path_ok(ix, n) ? PATH_SMALL : PATH_PHASES;
    run_batch<uint64_t, uint64_t>(ix, n, bytes, offs, hit_offs, false, err, out, out ? cap : 0, false);
    std::lock_guard<std::mutex> g(g_mu);
    g_counts.match++;
    return hipSuccess;
}

hipError_t launch_match_pairs(const DevIndex &ix, const Workspace &, uint64_t n, const uint8_t *bytes, const uint64_t *offs,
                              uint8_t *err, uint32_t *pairs, uint32_t *out, uint64_t cap, hipStream_t, hipEvent_t, hipEvent_t) {
    note_view(ix);
    if (!n) { pairs[0] = pairs[1] = 0; return hipSuccess; }
    run_batch<uint64_t, uint32_t>(ix, n, bytes, offs, pairs, true, err, out, out ? cap : 0, true);
    std::lock_guard<std::mutex> g(g_mu);
    g_counts.pairs++;
    return hipSuccess;
}

hipError_t launch_first(const DevIndex &ix, const Workspace &, uint64_t n, const uint8_t *bytes, const uint64_t *offs,
                        uint32_t *out_value, uint8_t *out_found, hipStream_t) {
    note_view(ix);
    imgw::UseStats st;
    imgw::Walker w(ix, st);
    std::vector<uint32_t> vals;
    for (uint64_t t = 0; t < n; t++) {
        vals.clear();
        const int e = w.match(bytes + offs[t], (uint32_t)(offs[t + 1] - offs[t]), vals);
        out_value[t] = !e && !vals.empty() ? vals[0] : 0;
        out_found[t] = e == 1 ? 2 : e == 2 ? 3 : !vals.empty();
    }
    std::lock_guard<std::mutex> g(g_mu);
    g_counts.first++;
    return hipSuccess;
}

hipError_t launch_small_segs(const DevIndex &ix, const Workspace &, const SmallSegs &sg, bool u32, uint32_t, LbCtl, int,
                             hipStream_t, int *path) {
    if (!sg.count || sg.count > (uint32_t)SMALL_SEGS) return hipErrorInvalidValue;
    if (sg.pairs && !u32) return hipErrorInvalidValue;
    note_view(ix);
    if (path) *path = PATH_SMALL;
    for (uint32_t k = 0; k < sg.count; k++) {
        const SmallSeg &s = sg.s[k];
        if (!s.n) return hipErrorInvalidValue;
        if (u32)
            run_batch<uint32_t, uint32_t>(ix, s.n, s.blob, static_cast<const uint32_t *>(s.offs), static_cast<uint32_t *>(s.hit),
                                          sg.pairs != 0, s.err, s.out, s.out ? s.cap : 0, false);
        else
            run_batch<uint64_t, uint64_t>(ix, s.n, s.blob, static_cast<const uint64_t *>(s.offs), static_cast<uint64_t *>(s.hit),
                                          false, s.err, s.out, s.out ? s.cap : 0, false);
    }
    std::lock_guard<std::mutex> g(g_mu);
    g_counts.small_segs++;
    return hipSuccess;
}

// k_patch: run r copies r.n words from data + r.src to word (r.dst & PATCH_OFF) of table (r.dst >> 48)
hipError_t launch_patch(const PatchRun *runs, const uint32_t *data, uint64_t n, PatchBases bases, hipStream_t) {
    for (uint64_t i = 0; i < n; i++) {
        const PatchRun &r = runs[i];
        const uint64_t table = r.dst >> 48, word = r.dst & PATCH_OFF;
        if (table >= (uint64_t)N_TABLES) imgw::die("patch run %llu names table %llu", (unsigned long long)i, (unsigned long long)table);
        uint8_t *dst = reinterpret_cast<uint8_t *>(bases.b[table]) + 4 * word;
        if (!bases.b[table] || fake_hip_room(dst) < 4ull * r.n)
            imgw::die("patch run %llu: words [%llu, +%u) of table %llu leave its device allocation", (unsigned long long)i,
                      (unsigned long long)word, r.n, (unsigned long long)table);
        memcpy(dst, data + r.src, 4ull * r.n);
    }
    std::lock_guard<std::mutex> g(g_mu);
    g_counts.patch++;
    g_counts.patch_runs += n;
    return hipSuccess;
}

// ---- matches_filter/3: the ordered walk over the rank-coded keys, per query

namespace {
struct Seek { uint64_t key; uint32_t pos, w; bool fin; };   // the first pos ranks of `key`, then w if fin
int cmp_key(const uint32_t *pool, const uint64_t *koff, uint64_t k, const Seek &s) {
    const uint64_t a0 = koff[k], klen = koff[k + 1] - a0, b0 = s.key == ~0ull ? 0 : koff[s.key];
    const uint64_t slen = (uint64_t)s.pos + (s.fin ? 1 : 0);
    for (uint64_t i = 0; i < std::min(klen, slen); i++) {
        const uint32_t a = pool[a0 + i], b = i < s.pos ? pool[b0 + i] : s.w;
        if (a != b) return a < b ? -1 : 1;
    }
    return klen < slen ? -1 : klen > slen;
}
uint64_t first_not_below(const uint32_t *pool, const uint64_t *koff, uint64_t K, const Seek &s) {
    uint64_t lo = 0, hi = K;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (cmp_key(pool, koff, mid, s) < 0) lo = mid + 1; else hi = mid;
    }
    return lo;
}
enum : int64_t { FULL = -1, PREFIX = -2, LOWER = -3 };
// compare/3 with a filter as the query: ranks '#' 0, '+' 1, words above
int64_t compare(const uint32_t *key, uint32_t kl, const uint32_t *q, uint32_t nq) {
    int64_t lastplus = -1;
    for (uint32_t i = 0;; i++) {
        if (i == kl) return i == nq ? FULL : PREFIX;
        if (key[i] == 0 && i + 1 == kl) return FULL;
        if (i < nq && q[i] == 0 && i + 1 == nq) return FULL;
        if (i == nq) break;
        if (q[i] == 1) continue;
        if (key[i] == 1) { lastplus = i; continue; }
        if (key[i] == q[i]) continue;
        if (key[i] > q[i]) break;
        return i;
    }
    return lastplus >= 0 ? lastplus : LOWER;
}
}  // namespace

hipError_t launch_matches_filter(uint64_t n, const uint32_t *qoff, const uint32_t *qr, const uint32_t *qbase,
                                 const uint32_t *pool, const uint64_t *koff, const uint32_t *kval, uint64_t K, uint32_t *cnt,
                                 const uint64_t *hit, uint32_t *out, uint64_t cap, uint8_t *err, hipStream_t) {
    for (uint64_t t = 0; t < n; t++) {
        const uint32_t *q = qr + qoff[t];
        const uint32_t nq = qoff[t + 1] - qoff[t];
        uint64_t cur = first_not_below(pool, koff, K, Seek{~0ull, 0, qbase[t], qbase[t] != NONE});
        uint64_t o = hit ? hit[t] : 0, c = 0, steps = 0;
        while (cur < K) {
            if (steps++ > 2 * K + 64) { err[t] = 1; break; }
            const int64_t r = compare(pool + koff[cur], (uint32_t)(koff[cur + 1] - koff[cur]), q, nq);
            if (r == FULL) {
                if (hit && o < cap) out[o] = kval[cur];
                o++; c++; cur++;
            } else if (r == PREFIX) {
                cur++;
            } else if (r == LOWER) {
                break;
            } else {
                const uint64_t nx = first_not_below(pool, koff, K, Seek{cur, (uint32_t)r, q[r], true});
                cur = nx > cur ? nx : cur + 1;
            }
        }
        if (!hit) cnt[t] = (uint32_t)c;
    }
    std::lock_guard<std::mutex> g(g_mu);
    g_counts.mfilter++;
    return hipSuccess;
}

// ---- the sorted orders of tm_match_batch

hipError_t launch_sort_segments(const Workspace &, uint64_t n, const uint64_t *hit_offs, uint32_t *out, uint64_t cap, int unique,
                                uint32_t *ucnt, hipStream_t) {
    for (uint64_t t = 0; t < n; t++) {
        const uint64_t b = hit_offs[t], e = hit_offs[t + 1];
        if (e > cap) { if (ucnt) ucnt[t] = 0; continue; }   // segments past cap are left alone
        std::sort(out + b, out + e);
        uint64_t d = e - b;
        if (unique) {
            d = (uint64_t)(std::unique(out + b, out + e) - (out + b));
            std::fill(out + b + d, out + e, NONE);
        }
        if (ucnt) ucnt[t] = (uint32_t)d;
    }
    std::lock_guard<std::mutex> g(g_mu);
    g_counts.sort++;
    return hipSuccess;
}

hipError_t launch_copy_values(const uint64_t *hit_offs, uint64_t n, const uint32_t *src, uint32_t *dst, uint64_t cap, hipStream_t) {
    const uint64_t m = std::min(hit_offs[n], cap);
    if (m) memcpy(dst, src, 4 * m);
    return hipSuccess;
}

// ---- everything else: not in the fake

hipError_t launch_match32(const DevIndex &, const Workspace &, uint64_t, const uint8_t *, const uint32_t *, uint32_t *, uint8_t *,
                          uint32_t *, uint64_t, uint32_t, LbCtl, int, hipStream_t, int *) { return unsupported(); }
hipError_t launch_offs_widen(const uint32_t *, uint64_t *, uint64_t, hipStream_t) { return unsupported(); }
hipError_t launch_offs_narrow(const uint64_t *, uint32_t *, uint64_t, hipStream_t) { return unsupported(); }
hipError_t launch_merge_shards(uint32_t, uint64_t, const uint64_t *, const uint32_t *, uint64_t, uint64_t *, uint32_t *, uint64_t,
                               hipStream_t) { return unsupported(); }
hipError_t launch_fanout(const FanoutScratch &, uint64_t, const uint64_t *, const uint32_t *, uint64_t, const uint32_t *, uint64_t,
                         uint32_t, uint64_t *, uint32_t *, uint32_t *, hipStream_t) { return unsupported(); }
hipError_t launch_fanout_pairs(const FanoutScratch &, uint64_t, const uint32_t *, const uint32_t *, uint64_t, const uint32_t *,
                               uint64_t, uint32_t, uint64_t *, uint32_t *, uint32_t *, hipStream_t) { return unsupported(); }
hipError_t launch_fanout_one(uint64_t, const uint32_t *, const uint32_t *, uint64_t, const uint32_t *, uint64_t, uint32_t,
                             uint32_t *, uint32_t *, uint32_t *, uint64_t, uint32_t *, hipStream_t) { return unsupported(); }
hipError_t launch_aggre(const FanoutScratch &, uint32_t, const uint64_t *, const uint32_t *, const uint32_t *, uint64_t,
                        const uint32_t *, uint64_t, uint64_t *, uint32_t *, uint32_t *, hipStream_t) { return unsupported(); }
hipError_t launch_aggre_one(const uint32_t *, const uint32_t *, uint32_t, const uint32_t *, const uint32_t *, const uint32_t *,
                            uint64_t, uint32_t *, uint32_t *, uint32_t *, uint64_t, uint32_t *, hipStream_t) { return unsupported(); }
hipError_t launch_dispatch(const FanoutScratch &, uint32_t, const uint64_t *, uint32_t, const uint32_t *, const uint32_t *, uint64_t,
                           const uint32_t *, uint64_t, const uint32_t *, uint64_t, uint64_t *, uint64_t *, uint32_t *, uint32_t *,
                           uint32_t *, uint64_t, hipStream_t) { return unsupported(); }
hipError_t launch_dispatch_one(const uint32_t *, const uint32_t *, const uint32_t *, const uint32_t *, const uint32_t *,
                               const uint32_t *, const uint32_t *, uint32_t, uint32_t, const uint32_t *, uint64_t, const uint32_t *,
                               uint64_t, uint32_t *, uint32_t *, uint32_t *, uint64_t, uint64_t *, uint32_t *, uint32_t *, uint32_t *,
                               uint64_t, uint64_t, uint32_t *, hipStream_t) { return unsupported(); }
hipError_t launch_share_pick(const FanoutScratch &, uint32_t, const uint64_t *, const uint32_t *, const uint32_t *, uint64_t,
                             const uint32_t *, const uint32_t *, uint64_t, uint32_t, const uint32_t *, uint64_t, const uint32_t *,
                             uint64_t, const uint32_t *, uint64_t, uint32_t *, uint64_t *, uint32_t *, hipStream_t) { return unsupported(); }
hipError_t launch_share_one(const uint32_t *, const uint32_t *, const uint32_t *, uint32_t, const uint32_t *, const uint32_t *,
                            uint64_t, uint64_t, const uint32_t *, const uint32_t *, uint64_t, uint32_t, const uint32_t *, uint64_t,
                            const uint32_t *, uint64_t, const uint32_t *, uint64_t, uint32_t *, uint32_t *, uint32_t *, hipStream_t) {
    return unsupported();
}
hipError_t launch_group_subs(const FanoutScratch &, const uint64_t *, const uint32_t *, const uint32_t *, const uint32_t *, uint64_t,
                             uint64_t *, uint32_t *, uint64_t *, uint64_t, uint32_t *, uint32_t *, uint32_t *, uint32_t *,
                             hipStream_t) { return unsupported(); }
hipError_t launch_group_picks(const FanoutScratch &, const uint64_t *, const uint32_t *, const uint32_t *, const uint32_t *, uint64_t,
                              uint32_t, const uint64_t *, const uint32_t *, const uint32_t *, const uint32_t *, uint64_t,
                              const uint32_t *, uint64_t, uint64_t *, uint32_t *, uint64_t *, uint64_t, uint32_t *, uint32_t *,
                              uint32_t *, uint32_t *, uint64_t, uint32_t, hipStream_t) { return unsupported(); }
hipError_t launch_group_one(const uint32_t *, const uint64_t *, const uint32_t *, const uint32_t *, const uint32_t *, uint64_t,
                            uint64_t, uint64_t *, uint32_t *, uint32_t *, uint32_t *, uint64_t *, uint32_t *, uint32_t *, uint64_t,
                            uint32_t *, hipStream_t) { return unsupported(); }
hipError_t launch_pd_gate(const uint32_t *, const uint64_t *, const uint32_t *, uint32_t, const uint32_t *, uint64_t, uint64_t,
                          uint64_t, uint64_t, uint64_t, uint64_t *, uint32_t *, uint32_t *, hipStream_t) { return unsupported(); }
hipError_t launch_group_picks_one(const uint32_t *, const uint64_t *, const uint32_t *, const uint32_t *, const uint32_t *,
                                  const uint32_t *, uint32_t, const uint32_t *, const uint32_t *, const uint32_t *, const uint32_t *,
                                  uint64_t, uint64_t, uint64_t, uint32_t *, uint32_t *, uint32_t *, uint32_t *, uint64_t *,
                                  uint32_t *, uint32_t *, uint64_t, uint32_t *, hipStream_t) { return unsupported(); }

}  // namespace tmx
