// tm_host.cpp -- host side of libtmatch: the index compiler, the delta applier
// that keeps an HBM mirror of it current, and the C ABI of include/tmatch.h.
//
// The reference stores one ETS ordered_set key per (filter, ID)
// (apps/emqx/src/emqx_topic_index.erl:50-62, key construction
// apps/emqx/src/emqx_trie_search.erl:115-140).  Here every insert/delete is
// applied to host copies of the flat tables described in tm_layout.h; each
// table records which of its 4-byte words changed, and tm_sync() ships exactly
// those words to HBM with one pinned H2D copy + one scatter kernel, in stream
// order before the next batch.  Tables that grow or
// rehash are re-uploaded whole.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <map>
#include <unordered_map>
#include <unordered_set>
#include <set>
#include <vector>

#include "../../include/tmatch.h"
#include "tm_dev.h"
#include "tm_subs.h"
#include "tm_layout.h"

using namespace tmx;

namespace {

thread_local std::string g_last_error;

// ------------------------------------------------------------ dirty words

struct Dirty {
    std::vector<std::pair<uint64_t, uint64_t>> r;   // [lo, hi) in 4-byte words
    bool all = true;
    void add(uint64_t lo, uint64_t hi) {
        if (all || lo >= hi) return;
        if (!r.empty() && lo >= r.back().first && lo <= r.back().second) {
            r.back().second = std::max(r.back().second, hi);
            return;
        }
        r.push_back({lo, hi});
    }
    void set_all() { all = true; r.clear(); }
    void clear() { all = false; r.clear(); }
};

constexpr int MAX_REPLICAS = 16;  // device copies of one host image (tm_create_replicas: devices x copies)

// host vector + its HBM copy on every replica
template <class T>
struct Mirror {
    std::vector<T> h;
    T *d[MAX_REPLICAS] = {};
    uint64_t dcap = 0;   // elements allocated on each replica's device
    Dirty dirty;
    void touch(uint64_t i, uint64_t n = 1) {
        uint64_t lo = i * sizeof(T), hi = (i + n) * sizeof(T);
        dirty.add(lo / 4, (hi + 3) / 4);
    }
    uint64_t bytes() const { return h.size() * sizeof(T); }
};

struct NodeAux {
    uint32_t parent = NONE, wid = NONE, hash_cap = 0, exact_cap = 0;
    uint32_t depth = 0;                       // words on the path from the root
    uint32_t hash_roff = 0, exact_roff = 0;   // the runs' offsets in vals (the line may hold an inline value)
    uint8_t is_plus = 0;
    uint32_t bm = NONE;                       // word offset of its child bitmap in wbits (wide nodes)
    uint32_t hdesc = 0;                       // keys P/#/... ('#' not last) ending their walk here (NLIT_HDESC)
};

struct WordRef { const uint8_t *p; uint32_t n; int kind; };   // kind: 0 binary, 1 '+', 2 '#'

// literal children of a node (its nlit word also carries NLIT_HDESC and the annex flags)
inline uint32_t nlit_of(const Node &n) { return n.nlit & NLIT_MASK; }

}  // namespace

// Per-caller execution context.  Host-API callers (tm_match_batch /
// tm_first_batch) check one out of a pool, so concurrent callers -- every
// client process calls matches/3 at once in the reference, on a shared
// read_concurrency table (emqx_topic_index.erl:41-48) -- run their batches on
// their own streams with their own scratch and staging buffers, and wait for
// the GPU without holding the index lock.  Device-API callers
// (tm_match_batch_dev) get one per stream they pass, in a bounded LRU pool.
struct Lane {
    int r = 0;                // the replica whose tables this lane's batches read
    hipStream_t s = nullptr;
    bool owned = false;       // stream created by the library (host-API lane)
    bool busy = false;        // checked out by a host-API caller
    bool used = false;        // `done` has been recorded
    bool drained = false;     // `done` was seen complete since it was last recorded (no API call needed)
    hipEvent_t done = nullptr;   // after the lane's last batch: later patches wait for it
    uint64_t tick = 0;        // last use (LRU of device-API lanes)
    uint32_t tag = 0;         // launches on this workspace (the one-launch path's look-back tag)
    uint64_t waited = 0;      // the replica's patch (seq) this lane's stream last waited for
    Workspace w{};
    // host-API staging: mapped pinned buffers (*_dev = their device
    // addresses) and the HBM copies used for batches above ZC_TOPICS
    uint8_t *pin_in = nullptr, *pin_in_dev = nullptr; uint64_t pin_in_cap = 0;
    uint8_t *pin_out = nullptr, *pin_out_dev = nullptr; uint64_t pin_out_cap = 0;
    uint8_t *d_in = nullptr; uint64_t d_in_cap = 0;
    uint8_t *d_res = nullptr; uint64_t d_res_cap = 0;
    uint32_t *pin_vals = nullptr, *pin_vals_dev = nullptr; uint64_t pin_vals_cap = 0;
    uint32_t *d_vals = nullptr; uint64_t d_vals_cap = 0;   // sorted output: values sorted in HBM first
    uint64_t *d_o64 = nullptr, *d_h64 = nullptr; uint64_t d_o64_cap = 0, d_h64_cap = 0;   // 32-bit device API: widened offsets
    // route fan-out (tm_fanout_dev / tm_route_batch): the passes' tables and
    // triples; tm_route_batch's device results (topics, values, bucket offsets)
    FanoutScratch f{};
    uint32_t *d_ft = nullptr, *d_fv = nullptr; uint64_t d_ft_cap = 0, d_fv_cap = 0;
    uint64_t *d_fo = nullptr; uint64_t d_fo_cap = 0;
    // tm_route_batch32 in place: the match's pairs (its values go to d_vals) and
    // the one-launch kernels' status words (mapped pinned: DP1_ST_WORDS, then
    // the [M, T] of a tm_dispatch_batch32 the grid kernels finished, then
    // k_sh_one's SH1_ST_WORDS under tm_publish_batch32, then k_gs_one's
    // GS1_ST_WORDS and the [M, T, G, W] of a tm_deliver_batch32 the grid
    // kernels finished)
    uint32_t *d_pr = nullptr; uint64_t d_pr_cap = 0;
    uint32_t *fo1_h = nullptr, *fo1_d = nullptr;
    // TM_ROUTE_AGGRE: the aggregated device results of the grid kernels, and the
    // one-launch fan-out's status words in device memory (k_ag_one passes them
    // on; under tm_dispatch_batch32 into a second pair, which k_dp_one reads;
    // then, 8-byte aligned, the [M, T] k_dp_one leaves for k_gs_one under
    // tm_deliver_batch32 and the [G, W] of the grid grouping: FO1S_WORDS)
    uint32_t *d_at = nullptr, *d_av = nullptr; uint64_t d_at_cap = 0, d_av_cap = 0;
    uint64_t *d_ao = nullptr; uint64_t d_ao_cap = 0;
    uint32_t *fo1_s = nullptr;
    // tm_dispatch_batch: the local bucket's deliveries (topic, value, subscriber)
    uint32_t *d_dt = nullptr, *d_dv = nullptr, *d_ds = nullptr; uint64_t d_dt_cap = 0, d_dv_cap = 0, d_ds_cap = 0;
    // tm_publish_batch: the picked member of every kept entry, then the pick's two head words
    uint32_t *d_sm = nullptr; uint64_t d_sm_cap = 0;
    uint32_t *d_sk = nullptr; uint64_t d_sk_cap = 0;   // its two key words per topic
    // tm_deliver_batch: the deliveries grouped by subscriber, the groups' subscribers and offsets
    uint32_t *d_gt = nullptr, *d_gv = nullptr, *d_gs = nullptr; uint64_t d_gt_cap = 0, d_gv_cap = 0, d_gs_cap = 0;
    uint32_t *d_gsub = nullptr; uint64_t d_gsub_cap = 0;
    uint64_t *d_goff = nullptr; uint64_t d_goff_cap = 0;
};

// Patch log: a ring of the last PATCH_RING patches (numbered 1, 2, ... in the
// order they were collected).  A patch is one pinned [PatchRun x runs | u32
// data] buffer shared by every replica (one host image: collected once), and
// reaches each replica lazily -- when a batch is about to run there -- so a
// replica no batch is reading can take a patch at once while the others are
// still busy with theirs (tm_options.copies).  A slot is reused only once
// every replica has applied the patch it holds (a lagging replica is brought
// up on its patch stream then).
// 128 slots: a slot is reused only once every copy has taken its patch, and a
// copy no batch reads lags the others; with 16 slots and a route mirror's
// group commits (~12k/s on 3 copies) the reuse brought a lagging copy up and
// waited for it under the index lock, 25 us per commit (TM_HOST_TIMING)
constexpr int PATCH_RING = 128;
constexpr uint64_t PATCH_ZC_MAX = 64 << 10;   // patches up to this size are read in place by the patch kernel
struct PatchSlot {
    uint8_t *pin = nullptr; uint64_t pin_cap = 0;
    uint8_t *pin_dev = nullptr;               // its device address (mapped: small patches are read in place)
    uint64_t bytes = 0, nr = 0, seq = 0;      // the patch held: size, runs, number (0: none)
};

// One device copy of the tables.  Patches reach it on the stream of the batch
// that is about to read it, or on the replica's patch stream.  Replicas of one
// entry of tm_create_replicas' device list form a group (tm_options.copies
// copies of the tables on that device).
struct Replica {
    int device = 0, group = 0;
    hipStream_t ps = nullptr;                 // patch stream (a lagging replica brought up out of band)
    hipEvent_t last_patch = nullptr;          // event of its latest patch (every batch waits for it)
    uint8_t *pdev[PATCH_RING] = {}; uint64_t pdev_cap[PATCH_RING] = {};
    hipEvent_t pdone[PATCH_RING] = {}; bool ppending[PATCH_RING] = {};
    uint64_t applied = 0;                     // patches applied (== tm_index::patch_seq: up to date)
    uint64_t last_use = 0;                    // tick of its latest batch
    uint64_t batches = 0;                     // host-API batches served (tm_replica_stats)
};


constexpr int MAX_HOST_LANES = 16;   // concurrent host-API batches in flight, per replica
constexpr int MAX_DEV_LANES = 16;    // device-API streams with a workspace kept

// concurrent combined launches of small host batches (tm_index::cmb_leaders)
constexpr int CMB_LEADERS = 4;   // (2 / 3 / 6 measured: profiles/r4/combiner/; round 5: 2 / 3, profiles/r5/conc/leaders_*)

struct tm_index {
    // Two locks (order: mu, then img).  `mu` covers the device side: lanes,
    // the patch log, the replicas, pinned buffers, profiling.  `img` covers
    // the host image: the tables' host vectors and dirty sets, the key maps,
    // matches_filter's log.  tm_apply_deltas takes only `img`, so compiling a
    // syncer batch never blocks a match batch that has no delta to pick up: a
    // batch takes `img` only to collect deltas applied since the last one
    // (`img_dirty`), and otherwise launches on the device view cached then.
    std::mutex mu;
    std::mutex img;
    std::atomic<bool> img_dirty{true};
    bool view_ok = false;
    std::condition_variable cv;      // a host lane was released
    int nrep = 1, ngroups = 1;
    Replica rep[MAX_REPLICAS];
    uint64_t rr = 0;                 // round-robin among equally loaded replicas

    // vocab: live words, next fresh wid, per-wid reference count (trie edges +
    // exact-key levels) and slot, wids freed for reuse; a word nothing refers
    // to any more is erased, so churn through unique levels (client ids, UUIDs)
    // does not grow the tables
    Mirror<VocabEntry> vocab; uint64_t vcount = 0; uint32_t wid_next = 0;
    std::vector<uint32_t> wref, wslot, free_wids;
    Mirror<uint8_t> wpool; uint64_t wpool_dead = 0;   // bytes of erased long words (compacted later)
    Mirror<Node> nodes; std::vector<NodeAux> aux; std::vector<uint32_t> free_nodes; uint64_t live_nodes = 0;
    Mirror<CSlot> ctab; std::vector<uint32_t> free_ctab[33]; uint64_t nlinks = 0, ntables = 0;
    Mirror<uint32_t> vals; std::vector<uint32_t> free_blocks[33];
    Mirror<ExactEntry> exact; std::vector<uint32_t> xcap, xroff; uint64_t xcount = 0;
    Mirror<uint16_t> xfp;   // exact-table fingerprints, slot for slot (0 = empty)
    Mirror<uint32_t> wseq; uint64_t wseq_dead = 0;   // words of erased long exact keys
    Mirror<uint32_t> wbits; uint32_t wb_words = 0;   // wide nodes' child bitmaps, wb_words words each
    std::vector<uint32_t> free_wbits; std::set<uint32_t> wide;
    // the nodes annexed to the vocab entries' hint slots (tm_layout.h HINT_*;
    // NONE: slot unused), chosen among the wide nodes by annex_designate
    uint32_t anx[ANX_SLOTS] = {NONE, NONE};
    bool anx_dirty = false;   // a node turned wide / stopped being wide, or an annexed node's child count moved
    // literal edges per (level, wid) and distinct edge words per level: a wide
    // node whose children cover most of its level's words probes its child
    // table directly (its line's bitmap pointer NONE, wide_dense)
    std::unordered_map<uint64_t, uint32_t> lvl_edges;
    std::vector<uint32_t> lvl_distinct;
    bool dense_dirty = false;

    // levels a walk must resolve (DevIndex::depth / xlen_*): live nodes per
    // depth and live exact keys per level count
    std::vector<uint64_t> depth_cnt, xlen_cnt;

    std::unordered_set<std::string> dead;
    // matches_filter/3 (tm_matches_filter) keeps its own copy of the word-list
    // keys, in term order on the device.  It is built from a fuzzy snapshot
    // of the trie taken in short slices under `mu` plus the log of every
    // word-list key op since the snapshot began (replayed afterwards), and
    // follows the log from then on, so the index lock is held only for
    // slices of a few hundred microseconds and to swap the log -- never for a
    // sort, an upload or a GPU wait (matches_filter stalled every
    // match batch for a second at 10M keys).
    struct MfState {
        std::mutex mu;                        // one matches_filter call at a time (never taken by matching)
        bool log_on = false, log_lost = false;   // (under ix->img) ops logged since the snapshot / log dropped
        std::vector<std::pair<bool, std::string>> log;   // (insert?, key) -- under ix->img
        std::unordered_set<std::string> keys; // kind | value | filter of every word-list key (under mu)
        bool have_keys = false, dev_stale = true;
        std::atomic<size_t> nkeys{0};         // keys.size(), for the log bound (read under ix->img)
        std::vector<std::string> words;       // distinct binary words, byte order
        uint32_t *pool = nullptr, *val = nullptr; uint64_t *koff = nullptr, K = 0;
        uint64_t pcap = 0, vcap = 0, kcap = 0;
        uint32_t *q = nullptr; uint64_t qcap = 0;   // staging: query offsets, ranks, bases, counts
        uint8_t *err = nullptr; uint64_t *hit = nullptr; uint32_t *out = nullptr;
        uint64_t ecap = 0, ocap = 0, hcap = 0;
        hipStream_t s = nullptr;
        uint64_t snapshots = 0, slices = 0;   // diagnostics
    } mf;
    uint64_t n_wild = 0, n_exact = 0;
    uint64_t n_hdesc_keys = 0;       // '#'-not-last keys stored (DevIndex::hdesc)
    uint64_t uploads = 0, patch_bytes = 0;

    PatchSlot patch[PATCH_RING]; uint64_t patch_seq = 0;   // patches collected so far
    // Patches every batch queued from now on must see (<= patch_seq): a
    // collect by a batch publishes what it collects at once; tm_commit
    // publishes its patch only once a copy no batch is reading holds it.
    uint64_t pub_seq = 0;
    int serving[MAX_REPLICAS];       // per group: the copy tm_commit last published on (-1: none)
    // tm_commit's image changes not yet published: batches do not collect
    // them meanwhile (they were not applied before those batches were queued)
    std::atomic<int> img_hold{0};
    std::atomic<uint64_t> commits{0}, commit_waits{0}, commit_forced{0};
    DevIndex view[MAX_REPLICAS];     // each replica's device view as of the last collect_patch

    std::vector<std::unique_ptr<Lane>> lanes;
    uint64_t tick = 0;

    // value -> destination (tm_set_dests; NONE: never set, unrouted): the
    // host array under `dst_mu` (taken after `mu`; tm_set_dests takes it alone)
    // and one device copy per group (device entry), which takes the
    // entries changed since its last upload -- [lo, hi) -- in stream order
    // before the next fan-out that reads it (dest_upload)
    std::mutex dst_mu;
    std::vector<uint32_t> dest_h;
    struct DestDev {
        uint32_t *d = nullptr; uint64_t cap = 0, len = 0;   // allocated / valid entries
        uint64_t lo = 0, hi = 0;                            // host entries newer than the device's
        uint32_t *pin = nullptr; uint64_t pin_cap = 0;      // upload staging
        hipEvent_t ev = nullptr; bool ev_set = false;       // after the last upload: other streams' fan-outs wait
        hipStream_t ev_s = nullptr;
    } dest[MAX_REPLICAS];
    // value -> the caller's id of the route's topic filter (tm_set_route_filters;
    // NONE: no filter known, equal to nothing): kept exactly as the
    // destinations are, under the same lock (table_upload)
    std::vector<uint32_t> filt_h;
    DestDev filt[MAX_REPLICAS];
    // value -> local subscriber list (tm_set_subscribers): the pool and the
    // spans of tm_subs.h, each kept on the device as the two tables above are,
    // under the same lock; a dispatch takes both in one hold of it, the pool
    // first (subs_upload)
    SubPool subs_h;
    DestDev sub_pool[MAX_REPLICAS], sub_span[MAX_REPLICAS];
    // shared subscriptions (tm_set_share_slots / tm_set_share_members): value ->
    // slot as the tables above; the slots' member lists in a second pool of
    // tm_subs.h, whose spans become the first two words of the 16-byte slot
    // records (pos, cnt, n_local, meta) the device gathers; all under the same
    // lock, a pick takes the three in one hold of it (share_upload).  The
    // slots' state words live on the device alone, one array per group, UNDEF
    // where never set; it grows with its contents kept (share_state_grow).
    std::vector<uint32_t> share_slot_h, share_rec_h;
    SubPool share_h;
    DestDev share_slot[MAX_REPLICAS], share_rec[MAX_REPLICAS], share_pool[MAX_REPLICAS];
    struct ShareState { uint32_t *d = nullptr; uint64_t cap = 0; } share_state[MAX_REPLICAS];
    // share member id -> local subscriber id (tm_set_member_subs; NONE: not a
    // connection of this node): kept exactly as the destinations are, under
    // the same lock (table_upload)
    std::vector<uint32_t> msub_h;
    DestDev msub[MAX_REPLICAS];

    // caller buffers from tm_host_alloc (host address -> size, device address;
    // vram: TM_ALLOC_VRAM device memory, the same address on both sides)
    struct Pinned { uint8_t *host, *dev; uint64_t size; bool vram; };
    std::vector<Pinned> pinned;

    // reader epochs (tm_read_begin / tm_read_end / tm_epoch): the epoch
    // advances after each delta batch is applied; registered readers' epochs
    std::atomic<uint64_t> epoch{1};
    std::mutex ep_mu;
    uint64_t next_ticket = 1;
    std::map<uint64_t, uint64_t> readers;     // ticket -> epoch at tm_read_begin
    std::multiset<uint64_t> reader_epochs;

    // diagnostics (tm_profile_*)
    bool prof = false;
    struct ProfEv { hipEvent_t b0, w0, w1, b1; int device; };
    std::vector<ProfEv> prof_pending, prof_free;
    double prof_walk_ms = 0, prof_batch_ms = 0;
    uint64_t prof_batches = 0;

    // test hooks (tm_debug_set, under mu): the look-back control of the next
    // dbg_lb_launches one-launch batches, and the two-phase path forced for
    // large batches
    LbCtl dbg_lb{LB_SPINS, NONE, 0};
    // TM_DEBUG_SMALL_TICKET: k_walk_small's blocks take start-order tickets
    // (the default since round 6: forward progress by construction, measured
    // free -- a lone 4k batch 0.038 vs 0.040 ms, concurrent CSR callers
    // 3.6-3.7 vs 3.3e8, profiles/r6/ticket/)
    uint32_t small_ticket = 1;
    bool patch_zc = true;           // TM_DEBUG_PATCH_ZC: small patches read in place from pinned memory
    uint64_t dbg_lb_launches = 0;
    bool dbg_phases = false;        // TM_DEBUG_PHASES: small batches on the two-phase path too (tests)
    int small_kind = SMALL_AUTO;    // TM_DEBUG_SMALL_KERNEL: which one-launch kernel takes small batches
    std::atomic<uint64_t> failed_batches{0}, retried_batches{0};   // one-launch look-back failures seen / retried
    std::atomic<uint64_t> path_batches[PATH_COUNT] = {};             // match launches per kernel path
    // tm_route_batch32 batches whose fan-out k_fo_one completed / that the grid kernels or the staged path finished
    std::atomic<uint64_t> route_one{0}, route_grid{0};
    // tm_dispatch_batch32 calls k_dp_one completed / that the grid kernels or the staged path finished
    std::atomic<uint64_t> dispatch_one{0}, dispatch_grid{0};
    // tm_publish_batch32 calls k_sh_one picked for / that the grid pick or the staged path finished
    std::atomic<uint64_t> publish_one{0}, publish_grid{0};
    uint64_t dp1_max = DP1_DELIVERIES;   // TM_DEBUG_DP1_MAX: deliveries k_dp_one expands itself
    // tm_deliver_batch32 calls k_gs_one grouped / that the grid kernels or the staged path finished; the
    // digit passes k_gs_one ran / skipped (TM_DEBUG_GROUP_PASSES_*: added to the grid form's)
    std::atomic<uint64_t> deliver_one{0}, deliver_grid{0}, gs1_passes[2] = {};
    uint64_t gs1_max = GS1_DELIVERIES;   // TM_DEBUG_GS1_MAX: deliveries k_gs_one groups itself
    // tm_publish_deliver_batch32 calls the one-workgroup ending finished (k_gp_one merged and grouped, or the
    // gate found a capacity short and nothing moved) / that the grid kernels or the staged path finished
    std::atomic<uint64_t> publish_deliver_one{0}, publish_deliver_grid{0};
    uint64_t gp1_max = GP1_DELIVERIES;   // TM_DEBUG_GP1_MAX: merged deliveries k_gp_one takes itself
    // The host-batch combiner (small_combined): small in-place 32-bit batches
    // of concurrent callers queue here; up to cmb_leaders callers at a time
    // each take what is queued and run it as ONE k_walk_small launch
    // (TM_DEBUG_COMBINE: 0 = every batch its own launch)
    std::mutex cmb_mu;
    std::condition_variable cmb_gcv;  // a gathering leader waits here for more batches
    std::deque<struct SmallReq *> cmb_q;
    int cmb_running = 0;              // launches being prepared or in flight (at most cmb_leaders)
    int cmb_inflight = 0;             // host batches those launches carry
    int cmb_gathering = 0;            // leaders waiting in the gather window
    int cmb_hw = 0;                   // recent high-water mark of queued + in-flight batches
    uint64_t cmb_hw_ns = 0;           // when it was last reached
    std::atomic<int> cmb_leaders{CMB_LEADERS};
    std::atomic<int> cmb_gather_us{0};   // TM_DEBUG_CMB_GATHER
    std::atomic<int> cmb_spin_us{0};     // TM_DEBUG_CMB_SPIN: a waiting caller spins this long before it sleeps
    std::atomic<uint64_t> cmb_launches{0}, cmb_batches{0};
};

namespace {

// errors are kept per calling thread (tm_last_error): concurrent callers of
// one index each see their own
int fail(tm_index *, int code, const std::string &msg) {
    g_last_error = msg;
    return code;
}

#define HIPCHK(h, x)                                                                    \
    do {                                                                                \
        hipError_t e_ = (x);                                                            \
        if (e_ != hipSuccess)                                                           \
            return fail(h, TM_EDEVICE, std::string(#x ": ") + hipGetErrorString(e_));   \
    } while (0)

// ---------------------------------------------------------------- hashing

void pack8(const uint8_t *p, uint32_t n, uint32_t &b0, uint32_t &b1);

uint64_t word_hash(const uint8_t *p, uint32_t n) {
    if (n <= VINL) {
        uint32_t b0, b1;
        pack8(p, n, b0, b1);
        return word_hash_short(b0, b1, n);
    }
    uint64_t x = FNV_OFF;
    for (uint32_t i = 0; i < n; i++) x = (x ^ p[i]) * FNV_PRIME;
    return word_hash_finish(x, n);
}

uint32_t pow2_at_least(uint64_t x) {
    uint64_t c = 16;
    while (c < x) c <<= 1;
    return (uint32_t)c;
}

// ------------------------------------------------------------------ vocab

void pack8(const uint8_t *p, uint32_t n, uint32_t &b0, uint32_t &b1) {
    b0 = b1 = 0;
    for (uint32_t i = 0; i < n && i < 8; i++) (i < 4 ? b0 : b1) |= (uint32_t)p[i] << (8 * (i % 4));
}

bool vocab_eq(tm_index *ix, const VocabEntry &e, uint64_t h, const uint8_t *p, uint32_t n) {
    if (n <= VINL) {   // (the tag's upper bits are hints)
        uint32_t b0, b1;
        pack8(p, n, b0, b1);
        return vocab_short_eq(e.tag, e.b0, e.b1, n, b0, b1);
    }
    return e.tag == vocab_tag(h, n) && e.b1 == n && !memcmp(ix->wpool.h.data() + e.b0, p, n);
}

uint32_t vocab_find(tm_index *ix, const uint8_t *p, uint32_t n) {
    const uint64_t h = word_hash(p, n);
    const uint32_t mask = (uint32_t)ix->vocab.h.size() - 1;
    for (uint32_t s = (uint32_t)h & mask;; s = (s + 1) & mask) {
        const VocabEntry &e = ix->vocab.h[s];
        if (e.wid == NONE) return NONE;
        if (vocab_eq(ix, e, h, p, n)) return e.wid;
    }
}

VocabEntry empty_vocab() { VocabEntry e; memset(&e, 0, sizeof e); e.wid = NONE; return e; }

// the word bytes of an entry (for rehashing)
void vocab_bytes(tm_index *ix, const VocabEntry &e, std::string &out) {
    uint32_t n = e.tag & 0xFF;
    if (n < VINL + 1) {
        out.resize(n);
        for (uint32_t i = 0; i < n; i++) out[i] = (char)(((i < 4 ? e.b0 : e.b1) >> (8 * (i % 4))) & 0xFF);
    } else {
        out.assign(reinterpret_cast<const char *>(ix->wpool.h.data() + e.b0), e.b1);
    }
}

constexpr uint32_t VOCAB_LOAD_SHIFT = 2;   // vocab load <= 1/4
uint64_t vocab_entry_hash(tm_index *ix, const VocabEntry &e) {
    std::string w;
    vocab_bytes(ix, e, w);
    return word_hash(reinterpret_cast<const uint8_t *>(w.data()), (uint32_t)w.size());
}

void vocab_rehash(tm_index *ix, uint64_t cap) {
    std::vector<VocabEntry> nt(cap, empty_vocab());
    const uint32_t mask = (uint32_t)nt.size() - 1;
    for (const VocabEntry &e : ix->vocab.h) {
        if (e.wid == NONE) continue;
        const uint64_t h = vocab_entry_hash(ix, e);
        for (uint32_t s = (uint32_t)h & mask;; s = (s + 1) & mask)
            if (nt[s].wid == NONE) { nt[s] = e; ix->wslot[e.wid] = s; break; }
    }
    ix->vocab.h.swap(nt);
    ix->vocab.dirty.set_all();
}

void wide_cover(tm_index *ix);

void vocab_grow(tm_index *ix, uint64_t need) {
    // load <= 1/4: the walk's deferred probes resolve on the first slot
    // almost always (one round trip per topic for all its levels)
    if ((need << VOCAB_LOAD_SHIFT) <= ix->vocab.h.size()) return;
    vocab_rehash(ix, pow2_at_least(need << VOCAB_LOAD_SHIFT));
}

uint32_t vocab_intern(tm_index *ix, const uint8_t *p, uint32_t n) {
    uint32_t w = vocab_find(ix, p, n);
    if (w != NONE) return w;
    vocab_grow(ix, ix->vcount + 1);
    VocabEntry e = empty_vocab();
    const uint64_t h = word_hash(p, n);
    e.tag = vocab_tag(h, n);
    if (!ix->free_wids.empty()) { e.wid = ix->free_wids.back(); ix->free_wids.pop_back(); }
    else {
        e.wid = ix->wid_next++;
        ix->wref.push_back(0);
        ix->wslot.push_back(NONE);
        wide_cover(ix);
    }
    if (n <= VINL) {
        pack8(p, n, e.b0, e.b1);
    } else {
        uint64_t off = ix->wpool.h.size();
        ix->wpool.h.resize(off + ((n + 3) & ~3u), 0);
        memcpy(ix->wpool.h.data() + off, p, n);
        ix->wpool.touch(off, (n + 3) & ~3u);
        e.b0 = (uint32_t)off;
        e.b1 = n;
    }
    const uint32_t mask = (uint32_t)ix->vocab.h.size() - 1;
    for (uint32_t s = (uint32_t)h & mask;; s = (s + 1) & mask)
        if (ix->vocab.h[s].wid == NONE) { ix->vocab.h[s] = e; ix->vocab.touch(s); ix->wslot[e.wid] = s; break; }
    ix->vcount++;
    return e.wid;
}

// the last trie edge / exact key using word `wid` is gone: erase it
// (backward-shift deletion, as ctab_erase) and free its wid and wpool bytes
void vocab_erase(tm_index *ix, uint32_t wid) {
    auto &t = ix->vocab.h;
    const uint32_t mask = (uint32_t)t.size() - 1;
    uint32_t i = ix->wslot[wid];
    if (t[i].wid != wid) return;   // never: wslot tracks every move
    if ((t[i].tag & 0xFF) > VINL) ix->wpool_dead += (t[i].b1 + 3) & ~3u;
    for (uint32_t j = (i + 1) & mask; t[j].wid != NONE; j = (j + 1) & mask) {
        const uint32_t k = (uint32_t)vocab_entry_hash(ix, t[j]) & mask;
        const bool stays = (i <= j) ? (i < k && k <= j) : (i < k || k <= j);
        if (!stays) { t[i] = t[j]; ix->wslot[t[i].wid] = i; ix->vocab.touch(i); i = j; }
    }
    t[i] = empty_vocab();
    ix->vocab.touch(i);
    ix->wslot[wid] = NONE;
    ix->free_wids.push_back(wid);
    ix->vcount--;
}

void word_ref(tm_index *ix, uint32_t wid) { ix->wref[wid]++; }
void word_unref(tm_index *ix, uint32_t wid) {
    if (--ix->wref[wid] == 0) vocab_erase(ix, wid);
}

// ------------------------------------------------- private child tables

uint32_t cls_of(uint32_t cap);

uint32_t ctab_alloc(tm_index *ix, uint32_t cap) {
    auto &fl = ix->free_ctab[cls_of(cap)];
    uint32_t o;
    if (!fl.empty()) { o = fl.back(); fl.pop_back(); }
    else { o = (uint32_t)ix->ctab.h.size(); ix->ctab.h.resize(o + cap); }
    for (uint32_t i = 0; i < cap; i++) ix->ctab.h[o + i] = CSlot{NONE, NONE, 0, 0};
    ix->ctab.touch(o, cap);
    ix->ntables++;
    return o;
}

void ctab_free(tm_index *ix, uint32_t off, uint32_t cap) {
    ix->free_ctab[cls_of(cap)].push_back(off);
    ix->ntables--;
}

void ctab_put(tm_index *ix, uint32_t off, uint32_t mask, uint32_t wid, uint32_t child, uint64_t sum) {
    for (uint32_t s = child_hash(wid) & mask;; s = (s + 1) & mask)
        if (ix->ctab.h[off + s].wid == NONE) {
            ix->ctab.h[off + s] = CSlot{wid, child, (uint32_t)sum, (uint32_t)(sum >> 32)};
            ix->ctab.touch(off + s);
            return;
        }
}

uint32_t ctab_find(tm_index *ix, uint32_t off, uint32_t mask, uint32_t wid) {
    for (uint32_t s = child_hash(wid) & mask;; s = (s + 1) & mask) {
        const CSlot &c = ix->ctab.h[off + s];
        if (c.wid == NONE) return NONE;
        if (c.wid == wid) return s;
    }
}

// backward-shift deletion inside one private table
void ctab_erase(tm_index *ix, uint32_t off, uint32_t mask, uint32_t wid) {
    uint32_t i = ctab_find(ix, off, mask, wid);
    if (i == NONE) return;
    CSlot *t = ix->ctab.h.data() + off;
    for (uint32_t j = (i + 1) & mask; t[j].wid != NONE; j = (j + 1) & mask) {
        uint32_t k = child_hash(t[j].wid) & mask;
        bool stays = (i <= j) ? (i < k && k <= j) : (i < k || k <= j);
        if (!stays) { t[i] = t[j]; ix->ctab.touch(off + i); i = j; }
    }
    t[i] = CSlot{NONE, NONE, 0, 0};
    ix->ctab.touch(off + i);
}

// ------------------------------------------------------------- value runs

uint32_t cls_of(uint32_t cap) { uint32_t c = 0; while ((1u << c) < cap) c++; return c; }

uint32_t val_alloc(tm_index *ix, uint32_t cap) {
    auto &fl = ix->free_blocks[cls_of(cap)];
    if (!fl.empty()) { uint32_t o = fl.back(); fl.pop_back(); return o; }
    uint64_t o = ix->vals.h.size();
    ix->vals.h.resize(o + cap, 0);
    return (uint32_t)o;
}

void val_free(tm_index *ix, uint32_t off, uint32_t cap) {
    if (cap) ix->free_blocks[cls_of(cap)].push_back(off);
}

// insert v into the sorted run (off, cnt) of capacity cap; false if present
bool run_insert(tm_index *ix, uint32_t &off, uint32_t &cnt, uint32_t &cap, uint32_t v) {
    uint32_t *b = ix->vals.h.data() + off;
    uint32_t pos = (uint32_t)(std::lower_bound(b, b + cnt, v) - b);
    if (pos < cnt && b[pos] == v) return false;
    if (cnt == cap) {
        uint32_t ncap = cap ? cap * 2 : 1;
        uint32_t noff = val_alloc(ix, ncap);
        memmove(ix->vals.h.data() + noff, ix->vals.h.data() + off, sizeof(uint32_t) * cnt);
        val_free(ix, off, cap);
        off = noff; cap = ncap;
        ix->vals.touch(off, cnt);
    }
    uint32_t *r = ix->vals.h.data() + off;
    memmove(r + pos + 1, r + pos, sizeof(uint32_t) * (cnt - pos));
    r[pos] = v;
    cnt++;
    ix->vals.touch(off + pos, cnt - pos);
    return true;
}

bool run_erase(tm_index *ix, uint32_t &off, uint32_t &cnt, uint32_t &cap, uint32_t v) {
    uint32_t *b = ix->vals.h.data() + off;
    uint32_t pos = (uint32_t)(std::lower_bound(b, b + cnt, v) - b);
    if (pos >= cnt || b[pos] != v) return false;
    memmove(b + pos, b + pos + 1, sizeof(uint32_t) * (cnt - pos - 1));
    cnt--;
    if (pos < cnt) ix->vals.touch(off + pos, cnt - pos);
    if (!cnt) { val_free(ix, off, cap); off = 0; cap = 0; }
    return true;
}

// Insert or erase v in a run kept at host offset roff (capacity cap), then
// write the run's device encoding into (doff, dcnt): a single value inline.
bool run_op(tm_index *ix, bool ins, uint32_t &roff, uint32_t &cap, uint32_t &doff, uint32_t &dcnt, uint32_t v) {
    uint32_t off = roff, cnt = dcnt & RUN_CNT;
    const bool changed = ins ? run_insert(ix, off, cnt, cap, v) : run_erase(ix, off, cnt, cap, v);
    roff = off;
    if (cnt == 1) { doff = ix->vals.h[off]; dcnt = 1u | RUN_INLINE; }
    else { doff = off; dcnt = cnt; }
    return changed;
}

// ------------------------------------------------------------------ nodes

uint32_t node_new(tm_index *ix, uint32_t parent, uint32_t wid, bool is_plus) {
    uint32_t id;
    if (!ix->free_nodes.empty()) { id = ix->free_nodes.back(); ix->free_nodes.pop_back(); }
    else { id = (uint32_t)ix->nodes.h.size(); ix->nodes.h.emplace_back(); ix->aux.emplace_back(); }
    Node nd; memset(&nd, 0, sizeof nd); nd.plus = NONE;
    for (uint32_t k = 0; k < KINL; k++) { nd.kw[k] = NONE; nd.kc[k] = NONE; }
    ix->nodes.h[id] = nd;
    ix->nodes.touch(id);
    NodeAux a; a.parent = parent; a.wid = wid; a.is_plus = is_plus;
    a.depth = parent == NONE ? 0 : ix->aux[parent].depth + 1;
    ix->aux[id] = a;
    ix->live_nodes++;
    if (ix->depth_cnt.size() <= a.depth) ix->depth_cnt.resize(a.depth + 1, 0);
    ix->depth_cnt[a.depth]++;
    if (!is_plus && wid != NONE) word_ref(ix, wid);   // the edge parent -> id uses the word
    return id;
}

// literal child of `node` for word `wid`
uint32_t child_find(tm_index *ix, uint32_t node, uint32_t wid) {
    const Node &n = ix->nodes.h[node];
    if (nlit_of(n) <= KINL) {
        for (uint32_t k = 0; k < KINL; k++) if (n.kw[k] == wid) return n.kc[k];
        return NONE;
    }
    uint32_t s = ctab_find(ix, n.kw[0], n.kw[1], wid);
    return s == NONE ? NONE : ix->ctab.h[n.kw[0] + s].child;
}

void set_bloom(Node &n, uint32_t wid) {
    const uint32_t b = child_bit(child_hash(wid));
    bloom_word(n, b >> 5) |= 1u << (b & 31);
}

// ---- wide nodes' exact child bitmaps (tm_layout.h WIDE_LIT)

void wide_bit(tm_index *ix, uint32_t node, uint32_t wid, bool on) {
    const uint32_t bm = ix->aux[node].bm;
    if (bm == NONE) return;
    uint32_t &w = ix->wbits.h[bm + (wid >> 5)];
    if (on) w |= 1u << (wid & 31); else w &= ~(1u << (wid & 31));
    ix->wbits.touch(bm + (wid >> 5));
}

// (re)write node's bitmap from its child table and point the line at it
void wide_fill(tm_index *ix, uint32_t node) {
    const uint32_t bm = ix->aux[node].bm;
    std::fill(ix->wbits.h.begin() + bm, ix->wbits.h.begin() + bm + ix->wb_words, 0u);
    Node &n = ix->nodes.h[node];
    for (uint32_t i = 0; i <= n.kw[1]; i++) {
        const uint32_t w = ix->ctab.h[n.kw[0] + i].wid;
        if (w != NONE) ix->wbits.h[bm + (w >> 5)] |= 1u << (w & 31);
    }
    ix->wbits.touch(bm, ix->wb_words);
    n.kw[2] = bm;   // (wide_dense may point a dense node's line away from it again)
    ix->nodes.touch(node);
    ix->dense_dirty = true;
}

uint32_t wide_alloc(tm_index *ix) {
    if (!ix->free_wbits.empty()) { uint32_t o = ix->free_wbits.back(); ix->free_wbits.pop_back(); return o; }
    const uint32_t o = (uint32_t)ix->wbits.h.size();
    ix->wbits.h.resize(o + ix->wb_words, 0u);
    return o;
}

// bitmaps cover every wid handed out so far: grow them all (rare: the vocab
// doubles) before a new wid could be looked up in one
void wide_cover(tm_index *ix) {
    if (ix->wide.empty() || (uint64_t)ix->wb_words * 32 >= ix->wid_next) return;
    uint32_t words = std::max<uint32_t>(ix->wb_words, 1024);
    while ((uint64_t)words * 32 < ix->wid_next) words *= 2;
    ix->wb_words = words;
    ix->wbits.h.clear();
    ix->free_wbits.clear();
    for (uint32_t node : ix->wide) {
        ix->aux[node].bm = wide_alloc(ix);
        wide_fill(ix, node);
    }
    ix->wbits.dirty.set_all();
}

void to_wide(tm_index *ix, uint32_t node) {
    ix->anx_dirty = true;
    if (ix->wide.empty()) ix->wb_words = 0;
    ix->wide.insert(node);
    if ((uint64_t)ix->wb_words * 32 < ix->wid_next) {
        ix->aux[node].bm = NONE;
        wide_cover(ix);   // sizes the bitmaps and fills this node's too
        return;
    }
    ix->aux[node].bm = wide_alloc(ix);
    wide_fill(ix, node);
}

void annex_set(tm_index *ix, uint32_t s, uint32_t p);
int annex_slot(const tm_index *ix, uint32_t p);

void from_wide(tm_index *ix, uint32_t node) {
    if (const int s = annex_slot(ix, node); s >= 0) annex_set(ix, (uint32_t)s, NONE);
    ix->anx_dirty = true;
    ix->free_wbits.push_back(ix->aux[node].bm);
    ix->aux[node].bm = NONE;
    ix->wide.erase(node);
    Node &n = ix->nodes.h[node];
    for (uint32_t j = 0; j < 6; j++) bloom_word(n, j) = 0;
    for (uint32_t i = 0; i <= n.kw[1]; i++) {
        const uint32_t w = ix->ctab.h[n.kw[0] + i].wid;
        if (w != NONE) set_bloom(n, w);
    }
    ix->nodes.touch(node);
}

// literal-children Bloom of node q (PSUM_BLOOM bits), all ones past PSUM_BLOOM children
uint64_t lit_bloom(tm_index *ix, uint32_t q) {
    const Node &n = ix->nodes.h[q];
    uint64_t m = 0;
    auto add = [&](uint32_t wid) { m |= 1ull << psum_bit(child_hash(wid)); };
    if (nlit_of(n) <= KINL) {
        for (uint32_t k = 0; k < KINL; k++) if (n.kw[k] != NONE) add(n.kw[k]);
    } else if (nlit_of(n) > PSUM_BLOOM) {
        m = (1ull << PSUM_BLOOM) - 1;
    } else {
        for (uint32_t i = 0; i <= n.kw[1]; i++) if (ix->ctab.h[n.kw[0] + i].wid != NONE) add(ix->ctab.h[n.kw[0] + i].wid);
    }
    return m;
}

uint64_t node_flags(const Node &n) {
    return (n.hash_cnt ? PSUM_HASH : 0) | (n.exact_cnt ? PSUM_EXACT : 0) | (n.plus != NONE ? PSUM_PLUS : 0) |
           ((n.nlit & NLIT_HDESC) ? PSUM_HDESC : 0);
}

// summary of node q as its parent keeps it (tm_layout.h PSUM_*)
uint64_t node_psum(tm_index *ix, uint32_t q) {
    const Node &n = ix->nodes.h[q];
    uint64_t m = node_flags(n) | lit_bloom(ix, q) << PSUM_BQ;
    if (n.plus != NONE) m |= node_flags(ix->nodes.h[n.plus]) << PSUM_QQ | lit_bloom(ix, n.plus) << PSUM_BQQ;
    return m;
}

// node x changed: refresh its parent's summary of it -- the parent line's psum
// for a '+' child, the child-table slot for a literal child of a table-mode
// parent (inline-mode parents keep no per-child summary)
void summary_refresh1(tm_index *ix, uint32_t x);
void summary_refresh(tm_index *ix, uint32_t x) {
    // x's summary sits in its parent; the parent's own summary (in the
    // grandparent) covers x too when x is the parent's '+' child
    summary_refresh1(ix, x);
    if (x != ROOT && ix->aux[x].is_plus) summary_refresh1(ix, ix->aux[x].parent);
}

// ---- vocab-entry hints (tm_layout.h HINT_*)

// the hint slot node p is annexed to, or -1
int annex_slot(const tm_index *ix, uint32_t p) {
    for (uint32_t s = 0; s < ANX_SLOTS; s++) if (ix->anx[s] == p) return (int)s;
    return -1;
}

// write slot s's 12 bits of word wid's entry (short words only: a long word's
// tag is its hash, and the walk probes for it as without hints)
void hint_put(tm_index *ix, uint32_t s, uint32_t wid, uint32_t hint) {
    const uint32_t sl = ix->wslot[wid];
    if (sl == NONE) return;
    VocabEntry &e = ix->vocab.h[sl];
    if (e.wid != wid || (e.tag & 0xFFu) > VINL) return;
    const uint32_t sh = s ? HINT_SHIFT1 : HINT_SHIFT0;
    const uint32_t t = (e.tag & ~(HINT_MASK << sh)) | hint << sh;
    if (t != e.tag) { e.tag = t; ix->vocab.touch(sl); }
}

// The hint is a pure function of the child's slot in p's table, so it is
// written again from the slot wherever a slot of an annexed parent is put,
// erased or refreshed -- in the same delta batch, hence in the same patch (or
// before the same whole-table upload) as the slot itself.
void hint_sync(tm_index *ix, uint32_t p, uint32_t wid) {
    const int s = annex_slot(ix, p);
    if (s < 0) return;
    const Node &pn = ix->nodes.h[p];
    uint32_t hint = 0;
    if (nlit_of(pn) > KINL) {
        const uint32_t sl = ctab_find(ix, pn.kw[0], pn.kw[1], wid);
        if (sl != NONE) { const CSlot &c = ix->ctab.h[pn.kw[0] + sl]; hint = hint_of_sum(c.sum_lo, c.sum_hi); }
    }
    hint_put(ix, (uint32_t)s, wid, hint);
}

// (re)write slot s in every short word's entry from node p's table (p == NONE:
// the slot is released; its bits are left as they are -- no node carries its
// flag and no view names its depth, so nothing reads them -- and written again
// here when the slot is next given out).  Rare; ships the vocab whole.
void annex_set(tm_index *ix, uint32_t s, uint32_t p) {
    const uint32_t flag = s ? NLIT_ANX1 : NLIT_ANX0;
    const uint32_t old = ix->anx[s];
    if (old != NONE) { ix->nodes.h[old].nlit &= ~flag; ix->nodes.touch(old); }
    ix->anx[s] = p;
    if (p == NONE) return;
    const uint32_t sh = s ? HINT_SHIFT1 : HINT_SHIFT0;
    for (VocabEntry &e : ix->vocab.h)
        if (e.wid != NONE && (e.tag & 0xFFu) <= VINL) e.tag &= ~(HINT_MASK << sh);
    Node &pn = ix->nodes.h[p];
    for (uint32_t i = 0; i <= pn.kw[1]; i++) {
        const CSlot &c = ix->ctab.h[pn.kw[0] + i];
        if (c.wid == NONE) continue;
        VocabEntry &e = ix->vocab.h[ix->wslot[c.wid]];
        if ((e.tag & 0xFFu) <= VINL) e.tag |= hint_of_sum(c.sum_lo, c.sum_hi) << sh;
    }
    ix->vocab.dirty.set_all();
    pn.nlit |= flag;
    ix->nodes.touch(p);
}

// Choose the annexed nodes: the wide nodes (depth >= 1) with the most literal
// children.  Hysteresis: a slot's node is replaced only when it stopped being
// wide (from_wide released it) or a wide node that holds no slot has at least
// twice its children.  Run with wide_dense, before the next patch.
void annex_designate(tm_index *ix) {
    if (!ix->anx_dirty) return;
    ix->anx_dirty = false;
    for (int round = 0; round < (int)ANX_SLOTS; round++) {
        uint32_t best = NONE;   // the widest wide node that holds no slot
        for (uint32_t node : ix->wide) {
            if (ix->aux[node].depth < 1 || annex_slot(ix, node) >= 0) continue;
            if (best == NONE || nlit_of(ix->nodes.h[node]) > nlit_of(ix->nodes.h[best])) best = node;
        }
        if (best == NONE) return;
        uint32_t s = ANX_SLOTS;   // a free slot, else the slot whose node has the fewest children
        for (uint32_t k = 0; k < ANX_SLOTS && s == ANX_SLOTS; k++) if (ix->anx[k] == NONE) s = k;
        if (s == ANX_SLOTS) {
            s = nlit_of(ix->nodes.h[ix->anx[1]]) < nlit_of(ix->nodes.h[ix->anx[0]]) ? 1 : 0;
            if (nlit_of(ix->nodes.h[best]) < 2 * (uint64_t)nlit_of(ix->nodes.h[ix->anx[s]])) return;
        }
        annex_set(ix, s, best);
    }
}

void summary_refresh1(tm_index *ix, uint32_t x) {
    if (x == ROOT) return;
    const NodeAux &a = ix->aux[x];
    const uint32_t p = a.parent;
    Node &pn = ix->nodes.h[p];
    if (a.is_plus) {
        if (pn.plus != x) return;
        const uint64_t m = node_psum(ix, x);
        if (pn.psum_lo != (uint32_t)m || pn.psum_hi != (uint32_t)(m >> 32)) {
            pn.psum_lo = (uint32_t)m; pn.psum_hi = (uint32_t)(m >> 32);
            ix->nodes.touch(p);
        }
        return;
    }
    if (nlit_of(pn) <= KINL) return;
    const uint32_t sl = ctab_find(ix, pn.kw[0], pn.kw[1], a.wid);
    if (sl == NONE) return;
    CSlot &c = ix->ctab.h[pn.kw[0] + sl];
    if (c.child != x) return;
    const uint64_t m = node_psum(ix, x);
    if (c.sum_lo != (uint32_t)m || c.sum_hi != (uint32_t)(m >> 32)) {
        c.sum_lo = (uint32_t)m; c.sum_hi = (uint32_t)(m >> 32);
        ix->ctab.touch(pn.kw[0] + sl);
        hint_sync(ix, p, a.wid);
    }
}

// move a node's children into a private table of `cap` slots (cap = pow2)
void to_table(tm_index *ix, uint32_t node, uint32_t cap) {
    Node &n = ix->nodes.h[node];
    std::vector<CSlot> kids;
    if (nlit_of(n) <= KINL) {
        for (uint32_t k = 0; k < KINL; k++)
            if (n.kw[k] != NONE) {
                const uint64_t m = node_psum(ix, n.kc[k]);
                kids.push_back({n.kw[k], n.kc[k], (uint32_t)m, (uint32_t)(m >> 32)});
            }
    } else {
        for (uint32_t i = 0; i <= n.kw[1]; i++) if (ix->ctab.h[n.kw[0] + i].wid != NONE) kids.push_back(ix->ctab.h[n.kw[0] + i]);
        ctab_free(ix, n.kw[0], n.kw[1] + 1);
    }
    uint32_t off = ctab_alloc(ix, cap);
    Node &m = ix->nodes.h[node];
    for (uint32_t j = 0; j < 6; j++) bloom_word(m, j) = 0;
    for (auto &c : kids) {
        ctab_put(ix, off, cap - 1, c.wid, c.child, (uint64_t)c.sum_hi << 32 | c.sum_lo);
        set_bloom(m, c.wid);
    }
    m.kw[0] = off; m.kw[1] = cap - 1;
    if (ix->aux[node].bm != NONE) {   // wide: the bitmap, not the Bloom (wide_dense decides again)
        m.kw[2] = ix->aux[node].bm;
        ix->dense_dirty = true;
    }
}

// A literal edge with word `wid` appears at / leaves level `lvl`.
void lvl_edge(tm_index *ix, uint32_t lvl, uint32_t wid, bool add) {
    const uint64_t k = (uint64_t)lvl << 32 | wid;
    if (ix->lvl_distinct.size() <= lvl) ix->lvl_distinct.resize(lvl + 1, 0);
    if (add) {
        if (ix->lvl_edges[k]++ == 0) { ix->lvl_distinct[lvl]++; ix->dense_dirty |= !ix->wide.empty(); }
    } else {
        auto it = ix->lvl_edges.find(k);
        if (it != ix->lvl_edges.end() && --it->second == 0) {
            ix->lvl_edges.erase(it);
            ix->lvl_distinct[lvl]--;
            ix->dense_dirty |= !ix->wide.empty();
        }
    }
}

// Dense wide nodes.  A wide node's bitmap line answers "may w be a child?"
// before its child table is probed: one more L2 request in the chain of every
// visit, worth it only where the answer is often no.  C3's level-1 nodes and
// the root's '+' child have (nearly) every word of their level as a child, so
// their bitmap is pure overhead on almost every topic; there the line's
// bitmap pointer is NONE and the walk probes the table at once.  Dense: the
// node's children are at least DENSE_NUM/DENSE_DEN of the distinct words
// that appear as literal edges at its children's level anywhere in the trie
// (the words a topic reaching it is likely to carry there).  Re-evaluated for
// every wide node when an edge count changed, before the next patch.
constexpr uint64_t DENSE_NUM = 3, DENSE_DEN = 5;
void wide_dense(tm_index *ix) {
    if (!ix->dense_dirty) return;
    ix->dense_dirty = false;
    for (uint32_t node : ix->wide) {
        Node &n = ix->nodes.h[node];
        const uint32_t lvl = ix->aux[node].depth;
        const uint64_t distinct = lvl < ix->lvl_distinct.size() ? ix->lvl_distinct[lvl] : 0;
        const bool dense = (uint64_t)nlit_of(n) * DENSE_DEN >= distinct * DENSE_NUM;
        const uint32_t want = dense ? NONE : ix->aux[node].bm;
        if (n.kw[2] != want) { n.kw[2] = want; ix->nodes.touch(node); }
    }
}

void child_add(tm_index *ix, uint32_t node, uint32_t wid, uint32_t child) {
    ix->nlinks++;
    lvl_edge(ix, ix->aux[node].depth, wid, true);
    if (ix->aux[node].bm != NONE) { ix->dense_dirty = true; ix->anx_dirty = true; }
    Node *n = &ix->nodes.h[node];
    if (nlit_of(*n) < KINL) {
        for (uint32_t k = 0; k < KINL; k++)
            if (n->kw[k] == NONE) { n->kw[k] = wid; n->kc[k] = child; break; }
    } else {
        if (nlit_of(*n) == KINL) to_table(ix, node, 16);
        else if ((nlit_of(*n) + 1) * 2 > n->kw[1] + 1) to_table(ix, node, (n->kw[1] + 1) * 2);
        n = &ix->nodes.h[node];
        ctab_put(ix, n->kw[0], n->kw[1], wid, child, node_psum(ix, child));
        if (ix->aux[node].bm != NONE) wide_bit(ix, node, wid, true);
        else set_bloom(*n, wid);
        hint_sync(ix, node, wid);
    }
    n->nlit++;
    if (nlit_of(*n) == WIDE_LIT && ix->aux[node].bm == NONE) { to_wide(ix, node); n = &ix->nodes.h[node]; }
    ix->nodes.touch(node);
    summary_refresh(ix, node);
}

void child_remove(tm_index *ix, uint32_t node, uint32_t wid) {
    ix->nlinks--;
    lvl_edge(ix, ix->aux[node].depth, wid, false);
    if (ix->aux[node].bm != NONE) { ix->dense_dirty = true; ix->anx_dirty = true; }
    Node &n = ix->nodes.h[node];
    if (nlit_of(n) <= KINL) {
        for (uint32_t k = 0; k < KINL; k++)
            if (n.kw[k] == wid) { n.kw[k] = NONE; n.kc[k] = NONE; break; }
        n.nlit--;
    } else {
        ctab_erase(ix, n.kw[0], n.kw[1], wid);
        wide_bit(ix, node, wid, false);
        hint_sync(ix, node, wid);
        n.nlit--;
        if (ix->aux[node].bm != NONE && nlit_of(n) < WIDE_LIT) from_wide(ix, node);
        if (nlit_of(n) == KINL) {   // back to inline mode
            std::vector<CSlot> kids;
            for (uint32_t i = 0; i <= n.kw[1]; i++) if (ix->ctab.h[n.kw[0] + i].wid != NONE) kids.push_back(ix->ctab.h[n.kw[0] + i]);
            ctab_free(ix, n.kw[0], n.kw[1] + 1);
            for (uint32_t k = 0; k < KINL; k++) { n.kw[k] = kids[k].wid; n.kc[k] = kids[k].child; }
        }
    }
    ix->nodes.touch(node);
    summary_refresh(ix, node);
}

bool node_empty(tm_index *ix, uint32_t id) {
    const Node &n = ix->nodes.h[id];
    return n.plus == NONE && nlit_of(n) == 0 && n.hash_cnt == 0 && n.exact_cnt == 0 && ix->aux[id].hdesc == 0;
}

void node_prune(tm_index *ix, uint32_t id) {
    while (id != ROOT && node_empty(ix, id)) {
        NodeAux a = ix->aux[id];
        if (a.is_plus) {
            Node &pn = ix->nodes.h[a.parent];
            pn.plus = NONE; pn.psum_lo = pn.psum_hi = 0;
            ix->nodes.touch(a.parent);
            summary_refresh(ix, a.parent);
        } else {
            child_remove(ix, a.parent, a.wid);
            word_unref(ix, a.wid);
        }
        ix->free_nodes.push_back(id);
        ix->live_nodes--;
        ix->depth_cnt[a.depth]--;
        id = a.parent;
    }
}

// ------------------------------------------------------------ exact table

ExactEntry empty_exact() { ExactEntry e; memset(&e, 0, sizeof e); e.nlev = NONE; return e; }

uint64_t seq_hash(const std::vector<uint32_t> &w) {
    uint64_t x = FNV_OFF;
    for (uint32_t v : w) x = seq_hash_step(x, v);
    return seq_hash_finish(x, (uint32_t)w.size());
}

bool exact_eq(tm_index *ix, const ExactEntry &e, uint64_t h, const std::vector<uint32_t> &w) {
    if (e.h_lo != (uint32_t)h || e.h_hi != (uint32_t)(h >> 32) || e.nlev != w.size()) return false;
    const uint32_t *s = w.size() <= XINL ? e.wids : ix->wseq.h.data() + e.seq_off;
    return !memcmp(s, w.data(), sizeof(uint32_t) * w.size());
}

uint32_t exact_find_slot(tm_index *ix, uint64_t h, const std::vector<uint32_t> &w) {
    const uint32_t mask = (uint32_t)ix->exact.h.size() - 1;
    for (uint32_t s = (uint32_t)h & mask;; s = (s + 1) & mask) {
        const ExactEntry &e = ix->exact.h[s];
        if (e.nlev == NONE) return NONE;
        if (exact_eq(ix, e, h, w)) return s;
    }
}

void exact_rehash(tm_index *ix, uint32_t ncap);
void exact_grow(tm_index *ix, uint64_t need) {
    if (need * 2 <= ix->exact.h.size()) return;
    exact_rehash(ix, pow2_at_least(need * 2));
}

void exact_rehash(tm_index *ix, uint32_t ncap) {
    std::vector<ExactEntry> nt(ncap, empty_exact());
    std::vector<uint32_t> nc(ncap, 0), nr(ncap, 0);
    std::vector<uint16_t> nf(ncap, 0);
    const uint32_t mask = ncap - 1;
    for (size_t i = 0; i < ix->exact.h.size(); i++) {
        const ExactEntry &e = ix->exact.h[i];
        if (e.nlev == NONE) continue;
        for (uint32_t s = e.h_lo & mask;; s = (s + 1) & mask)
            if (nt[s].nlev == NONE) { nt[s] = e; nc[s] = ix->xcap[i]; nr[s] = ix->xroff[i]; nf[s] = ix->xfp.h[i]; break; }
    }
    ix->exact.h.swap(nt);
    ix->xcap.swap(nc);
    ix->xroff.swap(nr);
    ix->xfp.h.swap(nf);
    ix->exact.dirty.set_all();
    ix->xfp.dirty.set_all();
}

void exact_erase_slot(tm_index *ix, uint32_t i) {
    auto &t = ix->exact.h;
    const uint32_t mask = (uint32_t)t.size() - 1;
    {   // the key's levels no longer use their words
        const uint32_t nl = t[i].nlev;
        const uint32_t *ws = nl <= XINL ? t[i].wids : ix->wseq.h.data() + t[i].seq_off;
        std::vector<uint32_t> used(ws, ws + nl);
        if (nl > XINL) ix->wseq_dead += nl;
        for (uint32_t w : used) word_unref(ix, w);
        ix->xlen_cnt[nl]--;
    }
    for (uint32_t j = (i + 1) & mask; t[j].nlev != NONE; j = (j + 1) & mask) {
        uint32_t k = t[j].h_lo & mask;
        bool stays = (i <= j) ? (i < k && k <= j) : (i < k || k <= j);
        if (!stays) {
            t[i] = t[j]; ix->xcap[i] = ix->xcap[j]; ix->xroff[i] = ix->xroff[j]; ix->xfp.h[i] = ix->xfp.h[j];
            ix->exact.touch(i); ix->xfp.touch(i);
            i = j;
        }
    }
    t[i] = empty_exact();
    ix->xcap[i] = 0;
    ix->xroff[i] = 0;
    ix->xfp.h[i] = 0;
    ix->exact.touch(i);
    ix->xfp.touch(i);
    ix->xcount--;
}

// Reclaim what deletes left behind (end of every delta batch): long words'
// bytes in wpool and long exact keys' wid runs in wseq are compacted once half
// of the pool is dead; the vocab and exact tables shrink back when their load
// falls below 1/16 and 1/8 (they double at 1/4 and 1/2).  Each of these
// rewrites whole tables, so the next sync re-uploads them.
void reclaim(tm_index *ix) {
    if (ix->wpool_dead * 2 > ix->wpool.h.size() && ix->wpool.h.size() >= (64u << 10)) {
        std::vector<uint8_t> np;
        np.reserve(ix->wpool.h.size() - ix->wpool_dead);
        for (VocabEntry &e : ix->vocab.h) {
            if (e.wid == NONE || (e.tag & 0xFF) <= VINL) continue;
            const uint64_t off = np.size(), padded = (e.b1 + 3) & ~3u;
            np.insert(np.end(), ix->wpool.h.begin() + e.b0, ix->wpool.h.begin() + e.b0 + padded);
            e.b0 = (uint32_t)off;
        }
        ix->wpool.h.swap(np);
        ix->wpool_dead = 0;
        ix->wpool.dirty.set_all();
        ix->vocab.dirty.set_all();
    }
    if (ix->wseq_dead * 2 > ix->wseq.h.size() && ix->wseq.h.size() >= (16u << 10)) {
        std::vector<uint32_t> nq;
        nq.reserve(ix->wseq.h.size() - ix->wseq_dead);
        for (ExactEntry &e : ix->exact.h) {
            if (e.nlev == NONE || e.nlev <= XINL) continue;
            const uint64_t off = nq.size();
            nq.insert(nq.end(), ix->wseq.h.begin() + e.seq_off, ix->wseq.h.begin() + e.seq_off + e.nlev);
            e.seq_off = (uint32_t)off;
        }
        ix->wseq.h.swap(nq);
        ix->wseq_dead = 0;
        ix->wseq.dirty.set_all();
        ix->exact.dirty.set_all();
    }
    const uint64_t vmin = 1024;
    if (ix->vocab.h.size() > vmin && (ix->vcount << (VOCAB_LOAD_SHIFT + 2)) < ix->vocab.h.size())
        vocab_rehash(ix, std::max<uint64_t>(vmin, pow2_at_least(std::max<uint64_t>(ix->vcount, 1) << VOCAB_LOAD_SHIFT)));
    if (ix->exact.h.size() > 1024 && ix->xcount * 8 < ix->exact.h.size())
        exact_rehash(ix, std::max<uint32_t>(1024, pow2_at_least(ix->xcount * 2)));
}

// --------------------------------------------------------------- key ops

void split_words(const uint8_t *f, uint32_t len, std::vector<WordRef> &out) {
    out.clear();
    uint32_t s = 0;
    for (uint32_t i = 0; i <= len; i++) {
        if (i == len || f[i] == '/') {
            uint32_t n = i - s;
            int kind = (n == 1 && f[s] == '+') ? 1 : (n == 1 && f[s] == '#') ? 2 : 0;
            out.push_back({f + s, n, kind});
            s = i + 1;
        }
    }
}

std::string dead_key(const uint8_t *f, uint32_t len, uint32_t v, uint8_t flags) {
    std::string k;
    k.reserve(len + 5);
    k.push_back((char)flags);
    k.append(reinterpret_cast<const char *>(&v), 4);
    k.append(reinterpret_cast<const char *>(f), len);
    return k;
}

// matches_filter's log of word-list key ops (tm_index::MfState; caller holds
// ix->mu).  Unbounded growth between calls is cut: past a bound the log is
// dropped and the next call takes a new snapshot.
void mf_log(tm_index *ix, bool ins, const std::string &key) {
    auto &m = ix->mf;
    if (!m.log_on) return;
    if (m.log.size() >= std::max<size_t>(size_t(1) << 22, 2 * m.nkeys.load(std::memory_order_relaxed))) {
        m.log_on = false; m.log_lost = true;
        std::vector<std::pair<bool, std::string>>().swap(m.log);
        return;
    }
    m.log.emplace_back(ins, key);
}

// one insert (ins = true) or delete of the key make_key(Filter, V)
// An escaped word list (TM_KEY_WORDS | TM_KEY_ESCAPED): words split on '/',
// "\x" = the byte x; a word written "\+" / "\#" is a binary word, a bare
// "+" / "#" the wildcard.  -> (word bytes, wildcard?) per word.
void esc_words(const uint8_t *f, uint32_t len, std::vector<std::pair<std::string, bool>> &out) {
    out.clear();
    std::string cur;
    bool esc_any = false;
    auto push = [&]() {
        const bool wild = !esc_any && cur.size() == 1 && (cur[0] == '+' || cur[0] == '#');
        out.emplace_back(cur, wild);
        cur.clear();
        esc_any = false;
    };
    for (uint32_t i = 0; i < len; i++) {
        if (f[i] == '\\' && i + 1 < len) { cur.push_back((char)f[++i]); esc_any = true; }
        else if (f[i] == '/') push();
        else cur.push_back((char)f[i]);
    }
    push();
}

// the canonical escaped form of a word list ('/' and '\' escaped, binary
// "+" / "#" as "\+" / "\#")
std::string esc_join(const std::vector<std::pair<std::string, bool>> &w) {
    std::string o;
    for (size_t i = 0; i < w.size(); i++) {
        if (i) o.push_back('/');
        if (w[i].second) { o += w[i].first; continue; }
        if (w[i].first == "+" || w[i].first == "#") { o.push_back('\\'); o += w[i].first; continue; }
        for (char c : w[i].first) {
            if (c == '/' || c == '\\') o.push_back('\\');
            o.push_back(c);
        }
    }
    return o;
}

// a binary word no topic level can equal: "+" / "#" (a level exactly that is
// badarg) or one holding a '/'
bool word_never(const std::pair<std::string, bool> &w) {
    return !w.second && (w.first == "+" || w.first == "#" || w.first.find('/') != std::string::npos);
}

void word_key_op(tm_index *ix, bool ins, const std::vector<WordRef> &w, uint32_t v, const std::string &dk,
                 bool dead_done);

void key_op(tm_index *ix, bool ins, const uint8_t *f, uint32_t len, uint32_t v, uint8_t flags,
            std::vector<WordRef> &w, std::vector<uint32_t> &wids) {
    if ((flags & TM_KEY_ESCAPED) && !(flags & TM_KEY_EMPTY_LIST)) {
        std::vector<std::pair<std::string, bool>> ew;
        esc_words(f, len, ew);
        bool never = false;
        for (auto &x : ew) never |= word_never(x);
        if (!never) {   // plain words after all: the TM_KEY_WORDS key of the joined bytes
            std::string plain;
            for (size_t i = 0; i < ew.size(); i++) { if (i) plain.push_back('/'); plain += ew[i].first; }
            key_op(ix, ins, reinterpret_cast<const uint8_t *>(plain.data()), (uint32_t)plain.size(), v,
                   TM_KEY_WORDS, w, wids);
            return;
        }
        // never matches a topic: a key of the table for matches_filter/3 only --
        // but a '#' atom before its last word still steers the ordered walk at
        // the node of the words before it, if those are plain (NLIT_HDESC)
        const std::string canon = esc_join(ew);
        const std::string dk = dead_key(reinterpret_cast<const uint8_t *>(canon.data()), (uint32_t)canon.size(), v,
                                        TM_KEY_WORDS | TM_KEY_ESCAPED);
        if (ix->mf.log_on) mf_log(ix, ins, dk);
        if (ins ? !ix->dead.insert(dk).second : !ix->dead.erase(dk)) return;   // present / absent: no-op
        size_t hpos = ew.size();
        for (size_t i = 0; i + 1 < ew.size(); i++)
            if (ew[i].second && ew[i].first == "#") { hpos = i; break; }
        bool plain_prefix = hpos < ew.size();
        for (size_t i = 0; i < hpos && plain_prefix; i++) plain_prefix = !word_never(ew[i]);
        if (!plain_prefix) return;
        std::vector<WordRef> pw;   // the prefix, the '#', and a stand-in for the rest (only the prefix is walked)
        for (size_t i = 0; i <= hpos; i++)
            pw.push_back({reinterpret_cast<const uint8_t *>(ew[i].first.data()), (uint32_t)ew[i].first.size(),
                          ew[i].second ? (ew[i].first == "+" ? 1 : 2) : 0});
        pw.push_back({nullptr, 0, 0});
        word_key_op(ix, ins, pw, v, dk, true);
        return;
    }
    if (flags & TM_KEY_EMPTY_LIST) {   // [] never matches a topic (topics have >= 1 level)
        auto k = dead_key(nullptr, 0, v, TM_KEY_EMPTY_LIST);
        if (ins) ix->dead.insert(k); else ix->dead.erase(k);
        mf_log(ix, ins, k);
        return;
    }
    split_words(f, len, w);
    bool wild = false;
    for (auto &x : w) wild |= x.kind != 0;
    if (!wild && !(flags & TM_KEY_WORDS)) {
        // binary key (emqx_trie_search.erl:121-125) -> exact table keyed by wid sequence
        wids.clear();
        if (ins) {
            for (auto &x : w) wids.push_back(vocab_intern(ix, x.p, x.n));
            exact_grow(ix, ix->xcount + 1);
        } else {
            for (auto &x : w) {
                uint32_t id = vocab_find(ix, x.p, x.n);
                if (id == NONE) return;
                wids.push_back(id);
            }
        }
        const uint64_t h = seq_hash(wids);
        uint32_t s = exact_find_slot(ix, h, wids);
        if (s == NONE) {
            if (!ins) return;
            ExactEntry e = empty_exact();
            e.h_lo = (uint32_t)h; e.h_hi = (uint32_t)(h >> 32); e.nlev = (uint32_t)wids.size();
            if (wids.size() <= XINL) {
                std::copy(wids.begin(), wids.end(), e.wids);
            } else {
                e.seq_off = (uint32_t)ix->wseq.h.size();
                ix->wseq.h.insert(ix->wseq.h.end(), wids.begin(), wids.end());
                ix->wseq.touch(e.seq_off, wids.size());
            }
            const uint32_t mask = (uint32_t)ix->exact.h.size() - 1;
            for (s = (uint32_t)h & mask; ix->exact.h[s].nlev != NONE; s = (s + 1) & mask) {}
            ix->exact.h[s] = e;
            ix->xcap[s] = 0;
            ix->xroff[s] = 0;
            ix->xfp.h[s] = exact_fp(h);
            ix->xfp.touch(s);
            ix->xcount++;
            for (uint32_t wd : wids) word_ref(ix, wd);
            if (ix->xlen_cnt.size() <= wids.size()) ix->xlen_cnt.resize(wids.size() + 1, 0);
            ix->xlen_cnt[wids.size()]++;
        }
        ExactEntry &e = ix->exact.h[s];
        if (ins) { if (run_op(ix, true, ix->xroff[s], ix->xcap[s], e.val_off, e.val_cnt, v)) ix->n_exact++; }
        else if (run_op(ix, false, ix->xroff[s], ix->xcap[s], e.val_off, e.val_cnt, v)) {
            ix->n_exact--;
            if (!(e.val_cnt & RUN_CNT)) { exact_erase_slot(ix, s); return; }
        }
        ix->exact.touch(s);
        return;
    }
    word_key_op(ix, ins, w, v, dead_key(f, len, v, TM_KEY_WORDS), false);
}

// A word-list key (its words w; dk: its dead-key string, the identity
// matches_filter/3 and the never-matching set know it by; dead_done: the
// caller already logged it and entered it in that set).
void word_key_op(tm_index *ix, bool ins, const std::vector<WordRef> &w, uint32_t v, const std::string &dk,
                 bool dead_done) {
    if (ix->mf.log_on && !dead_done) mf_log(ix, ins, dk);
    // word-list key.  '#' anywhere but last never matches (compare/3 has no
    // clause for it, emqx_trie_search.erl:282-290 vs :341-348; emqx_topic.erl:110),
    // but the key still steers the reference's walk at the node P of its
    // prefix before that '#' (tm_layout.h NLIT_HDESC): P counts such keys
    size_t hpos = w.size();
    for (size_t i = 0; i + 1 < w.size(); i++)
        if (w[i].kind == 2) { hpos = i; break; }
    if (hpos < w.size() && !dead_done) {
        // (a wildcard filter is a word list whatever the flag: one key)
        if (ins ? !ix->dead.insert(dk).second : !ix->dead.erase(dk)) return;   // present / absent: no-op
    }
    const bool hash_term = hpos == w.size() && w.back().kind == 2;
    const size_t end = hpos < w.size() ? hpos : hash_term ? w.size() - 1 : w.size();
    uint32_t node = ROOT;
    for (size_t i = 0; i < end; i++) {
        if (w[i].kind == 1) {
            uint32_t c = ix->nodes.h[node].plus;
            if (c == NONE) {
                if (!ins) return;
                c = node_new(ix, node, NONE, true);
                ix->nodes.h[node].plus = c;
                ix->nodes.touch(node);
                summary_refresh(ix, node);   // node gained a '+' child
                summary_refresh(ix, c);
            }
            node = c;
        } else {
            uint32_t wid = ins ? vocab_intern(ix, w[i].p, w[i].n) : vocab_find(ix, w[i].p, w[i].n);
            if (wid == NONE) return;
            uint32_t c = child_find(ix, node, wid);
            if (c == NONE) {
                if (!ins) return;
                c = node_new(ix, node, wid, false);
                child_add(ix, node, wid, c);
            }
            node = c;
        }
    }
    Node &nd = ix->nodes.h[node];
    NodeAux &a = ix->aux[node];
    if (hpos < w.size()) {   // a '#'-not-last key: P's count (the path exists: the key was inserted)
        a.hdesc += ins ? 1 : -1;
        ix->n_hdesc_keys += ins ? 1 : -1;
        nd.nlit = (nd.nlit & ~NLIT_HDESC) | (a.hdesc ? NLIT_HDESC : 0);
        ix->nodes.touch(node);
        summary_refresh(ix, node);
        if (!ins) node_prune(ix, node);
        return;
    }
    bool changed;
    changed = hash_term ? run_op(ix, ins, a.hash_roff, a.hash_cap, nd.hash_off, nd.hash_cnt, v)
                        : run_op(ix, ins, a.exact_roff, a.exact_cap, nd.exact_off, nd.exact_cnt, v);
    if (!changed) return;
    ix->nodes.touch(node);
    summary_refresh(ix, node);
    if (ins) ix->n_wild++;
    else { ix->n_wild--; node_prune(ix, node); }
}

// ------------------------------------------------------------- device side

constexpr uint64_t DEV_GUARD = 16;   // device elements kept allocated past the host size (see collect)

int bring_up(tm_index *ix, int r, uint64_t upto, hipStream_t st, bool idle = false);
int collect_patch_locked(tm_index *ix);

template <class T>
int upload_full(tm_index *ix, Mirror<T> &m) {
    // patches logged before this upload are older than it: every replica
    // takes them first (a lagging replica applying one later would write old
    // words over the new table)
    for (int r = 0; r < ix->nrep; r++)
        if (int rc = bring_up(ix, r, ix->patch_seq, ix->rep[r].ps)) return rc;
    uint64_t need = std::max<uint64_t>(m.h.size(), 1);
    // (collect's condition: a table within DEV_GUARD of its allocation grows, or every collect from
    // then on would ship it whole again, the guard shrinking to nothing, until it outgrew the allocation)
    const bool grow = need + DEV_GUARD > m.dcap;
    const uint64_t cap = grow ? need + need / 2 + DEV_GUARD : m.dcap;
    // a failure part way leaves the device copies in doubt: dcap 0 makes the
    // next collect reallocate and ship the whole table again (its dirty set
    // is cleared only on success)
    auto ship = [&]() -> int {
        for (int r = 0; r < ix->nrep; r++) {
            // rare (first upload, growth, rehash): drain every stream that may
            // still read the old copy before touching it
            HIPCHK(ix, hipSetDevice(ix->rep[r].device));
            HIPCHK(ix, hipDeviceSynchronize());
            if (grow) {
                if (m.d[r]) HIPCHK(ix, hipFree(m.d[r]));
                m.d[r] = nullptr;
                HIPCHK(ix, hipMalloc(&m.d[r], cap * sizeof(T)));
            }
            if (m.bytes()) HIPCHK(ix, hipMemcpy(m.d[r], m.h.data(), m.bytes(), hipMemcpyHostToDevice));
        }
        return TM_OK;
    };
    if (int rc = ship()) {
        m.dcap = 0;
        return rc;
    }
    m.dcap = cap;
    if (getenv("TM_DEBUG_UPLOADS"))   // diagnostics: which table was shipped whole, and why
        fprintf(stderr, "tm upload_full: %zu-byte elements x %zu (%.1f MB), dcap %lu, %d replicas\n", sizeof(T),
                m.h.size(), m.bytes() / 1e6, (unsigned long)m.dcap, ix->nrep);
    m.dirty.clear();
    ix->uploads++;
    return TM_OK;
}

// One patch run: `n` (<= PATCH_RUN) consecutive 4-byte words copied from the
// patch data at `src` to word `dst & PATCH_OFF` of table `dst >> 48` (tm_dev.h
// PatchRun): the same runs serve every replica, each with its table bases.
constexpr uint32_t PATCH_RUN = 64;

template <class T>
int collect(tm_index *ix, Mirror<T> &m, uint32_t table, std::vector<PatchRun> &runs, std::vector<uint32_t> &data) {
    // the device copy keeps >= DEV_GUARD elements allocated past the host
    // size: k_emit's 16-B loads may overhang the last value run by 3 words
    // (with h.size() == dcap such a load would leave the allocation)
    if (m.h.size() + DEV_GUARD > m.dcap) m.dirty.set_all();
    if (!m.dirty.all) {
        uint64_t words = 0;
        for (auto &r : m.dirty.r) words += r.second - r.first;
        if (words * 4 > m.bytes() / 2) m.dirty.set_all();   // cheaper to ship the table
    }
    if (m.dirty.all) return upload_full(ix, m);
    const uint8_t *src = reinterpret_cast<const uint8_t *>(m.h.data());
    const uint64_t limit = (m.bytes() + 3) / 4;
    for (auto &r : m.dirty.r) {
        const uint64_t hi = std::min<uint64_t>(r.second, limit);
        for (uint64_t lo = r.first; lo < hi; lo += PATCH_RUN) {
            const uint32_t n = (uint32_t)std::min<uint64_t>(PATCH_RUN, hi - lo);
            const uint64_t at = data.size();
            runs.push_back(PatchRun{(uint64_t)table << 48 | lo, (uint32_t)at, n});
            data.resize(at + n, 0);
            memcpy(data.data() + at, src + 4 * lo, std::min<uint64_t>(4ull * n, m.bytes() - 4 * lo));
        }
    }
    m.dirty.clear();
    return TM_OK;
}

PatchBases patch_bases(tm_index *ix, int r) {
    PatchBases b;
    const void *t[N_TABLES] = {ix->vocab.d[r], ix->wpool.d[r], ix->nodes.d[r], ix->ctab.d[r], ix->vals.d[r],
                               ix->exact.d[r], ix->xfp.d[r], ix->wseq.d[r], ix->wbits.d[r]};
    for (int i = 0; i < N_TABLES; i++) b.b[i] = reinterpret_cast<uint64_t>(t[i]);
    return b;
}

// a fresh launch tag of the lane's workspace (1 .. LB_TAG_MASK); when the tags
// wrap, the look-back words are cleared first, on the launch's stream, so no
// word an earlier launch left can carry the new tag
int next_tag(tm_index *ix, Lane &ln, hipStream_t s, uint32_t &tag) {
    ln.tag = (ln.tag + 1) & LB_TAG_MASK;
    if (!ln.tag) {
        ln.tag = 1;
        HIPCHK(ix, hipMemsetAsync(ln.w.look, 0, (ln.w.cap_n / SM_TOPICS + 4) * 8 * LB_STRIDE, s));
    }
    tag = ln.tag;
    return TM_OK;
}

// the look-back control of the next launch (caller holds ix->mu): the
// default bound, or the test hook's for the next dbg_lb_launches launches
LbCtl next_lb(tm_index *ix) {
    LbCtl c{LB_SPINS, NONE, 0};
    if (ix->dbg_lb_launches) {
        ix->dbg_lb_launches--;
        c = ix->dbg_lb;
    }
    c.ticket = ix->small_ticket;
    return c;
}

// did the lane's last one-launch batch fail its look-back (err 4, the fail
// word raised by the device)?  Clears the word.  After the lane's stream
// has been synchronised.
bool batch_failed(tm_index *ix, Lane &ln) {
    volatile uint32_t *f = ln.w.hint_h + HINT_FAIL;
    if (!*f) return false;
    *f = 0;
    ix->failed_batches++;
    return true;
}

// the lane's batch is done with the index: later patches (on any stream) wait for it
int batch_done(tm_index *ix, Lane &ln) {
    HIPCHK(ix, hipEventRecord(ln.done, ln.s));
    ln.used = true;
    ln.drained = false;
    return TM_OK;
}

// Is a batch of the lane still running?  (caller holds ix->mu)  A lane seen
// drained stays so until its next batch: the copy pickers, the committer and
// the patches ask about every lane under the index lock, and with concurrent
// callers that was dozens of event queries (and stream waits) per launch and
// per commit, while most lanes were long idle
bool lane_busy(Lane &l) {
    if (!l.used || l.drained) return false;
    if (hipEventQuery(l.done) == hipErrorNotReady) return true;
    l.drained = true;
    return false;
}

// Apply logged patch q to replica r on stream st.  Patches rewrite the tables
// in place, so a patch first waits for every batch still reading the replica
// (each of its lanes' `done`) and for the replica's patch before it; every
// later batch there waits for this one (`last_patch`, ensure_ws): a batch
// sees exactly the deltas applied before it was queued (C5), whichever stream
// either ran on.
int apply_patch(tm_index *ix, int r, uint64_t q, hipStream_t st, bool wait_readers = true) {
    Replica &R = ix->rep[r];
    const uint32_t k = (uint32_t)((q - 1) % PATCH_RING);
    const PatchSlot &p = ix->patch[k];
    HIPCHK(ix, hipSetDevice(R.device));
    // a small patch (a route write's few runs) is read by the patch kernel
    // straight from the mapped pinned slot: one command on the stream instead
    // of a DMA copy and the kernel behind it (the slot is reused only after
    // pdone, recorded behind the kernel); larger ones are copied first, into a
    // device buffer of the slot allocated on first use
    const bool zc = ix->patch_zc && p.pin_dev && p.bytes <= PATCH_ZC_MAX;
    if (!zc && (p.bytes > R.pdev_cap[k] || !R.pdev[k])) {
        if (R.ppending[k]) { HIPCHK(ix, hipEventSynchronize(R.pdone[k])); R.ppending[k] = false; }
        if (R.pdev[k]) HIPCHK(ix, hipFree(R.pdev[k]));
        R.pdev[k] = nullptr;
        R.pdev_cap[k] = 0;
        // generous steps: a reallocation (hipHostFree / hipFree) synchronises
        // the device, a multi-millisecond stall inside a churn stream (C5)
        const uint64_t want = std::max<uint64_t>(p.bytes * 2, 1u << 20);
        uint8_t *np = nullptr;   // the capacity is recorded only once the buffer exists
        HIPCHK(ix, hipMalloc(&np, want));
        R.pdev[k] = np;
        R.pdev_cap[k] = want;
    }
    if (wait_readers)   // (not for a copy known to be idle, nor again behind a patch just queued on st)
        for (auto &l : ix->lanes)
            if (l->r == r && l->s != st && lane_busy(*l)) HIPCHK(ix, hipStreamWaitEvent(st, l->done, 0));
    if (R.last_patch) HIPCHK(ix, hipStreamWaitEvent(st, R.last_patch, 0));
    const uint8_t *src = R.pdev[k];
    if (zc) {
        src = p.pin_dev;
    } else {
        HIPCHK(ix, hipMemcpyAsync(R.pdev[k], p.pin, p.bytes, hipMemcpyHostToDevice, st));
    }
    HIPCHK(ix, launch_patch(reinterpret_cast<const PatchRun *>(src),
                            reinterpret_cast<const uint32_t *>(src + p.nr * sizeof(PatchRun)), p.nr,
                            patch_bases(ix, r), st));
    HIPCHK(ix, hipEventRecord(R.pdone[k], st));
    R.ppending[k] = true;
    R.last_patch = R.pdone[k];
    R.applied = q;
    return TM_OK;
}

// replica r takes every logged patch up to `upto`, in order, on stream st
int bring_up(tm_index *ix, int r, uint64_t upto, hipStream_t st, bool idle) {
    const uint64_t first = ix->rep[r].applied + 1;   // (readers waited for once, before the first patch)
    for (uint64_t q = first; q <= upto; q++)
        if (int rc = apply_patch(ix, r, q, st, !idle && q == first)) return rc;
    return TM_OK;
}

DevIndex dev_view_build(tm_index *ix, int r);

// Collect every dirty word into a new logged patch and refresh the replicas'
// cached device views (caller holds ix->mu; takes ix->img, and only when a
// delta was applied since the last call); nothing reaches a device here but
// whole-table uploads
int collect_patch(tm_index *ix, bool commit = false) {
    if (ix->view_ok && !commit &&
        (!ix->img_dirty.load(std::memory_order_acquire) || ix->img_hold.load(std::memory_order_acquire) > 0))
        return TM_OK;
    std::lock_guard<std::mutex> gi(ix->img);
    ix->img_dirty.store(false, std::memory_order_relaxed);   // (an apply from here on sets it again)
    int rc = collect_patch_locked(ix);
    for (int r = 0; r < ix->nrep; r++) ix->view[r] = dev_view_build(ix, r);
    ix->view_ok = rc == TM_OK;
    if (!commit) ix->pub_seq = ix->patch_seq;   // a batch's collect: published at once
    return rc;
}

int collect_patch_locked2(tm_index *ix);

// Every table's dirty words go into one patch.  collect() clears a table's
// dirty set as it takes its runs, so if anything fails after that (a pinned
// allocation, a lagging replica's bring-up) those runs would never reach a
// device: every table is then marked wholly dirty, and the next collect ships
// them whole.
int collect_patch_locked(tm_index *ix) {
    const int rc = collect_patch_locked2(ix);
    if (rc) {
        ix->vocab.dirty.set_all(); ix->wpool.dirty.set_all(); ix->nodes.dirty.set_all();
        ix->ctab.dirty.set_all(); ix->vals.dirty.set_all(); ix->exact.dirty.set_all();
        ix->xfp.dirty.set_all(); ix->wseq.dirty.set_all(); ix->wbits.dirty.set_all();
    }
    return rc;
}

// (TM_HOST_TIMING) collect_patch_locked2's parts: the tables' runs, the ring
// slot's reuse (a lagging replica brought up and waited for), the pinned copy
std::atomic<uint64_t> g_col_n{0}, g_col_runs_ns{0}, g_col_slot_ns{0}, g_col_copy_ns{0};
const bool g_col_timing = getenv("TM_HOST_TIMING") != nullptr;
uint64_t col_now() {
    return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(
        std::chrono::steady_clock::now().time_since_epoch()).count();
}

int collect_patch_locked2(tm_index *ix) {
    const uint64_t t0 = g_col_timing ? col_now() : 0;
    std::vector<PatchRun> runs;
    std::vector<uint32_t> data;
    int rc;
    if ((rc = collect(ix, ix->vocab, 0, runs, data))) return rc;
    if ((rc = collect(ix, ix->wpool, 1, runs, data))) return rc;
    if ((rc = collect(ix, ix->nodes, 2, runs, data))) return rc;
    if ((rc = collect(ix, ix->ctab, 3, runs, data))) return rc;
    if ((rc = collect(ix, ix->vals, 4, runs, data))) return rc;
    if ((rc = collect(ix, ix->exact, 5, runs, data))) return rc;
    if ((rc = collect(ix, ix->xfp, 6, runs, data))) return rc;
    if ((rc = collect(ix, ix->wseq, 7, runs, data))) return rc;
    if ((rc = collect(ix, ix->wbits, 8, runs, data))) return rc;
    const uint64_t nr = runs.size(), nw = data.size();
    if (!nr) return TM_OK;
    const uint64_t t1 = g_col_timing ? col_now() : 0;
    const uint64_t q = ix->patch_seq + 1;
    const uint32_t k = (uint32_t)((q - 1) % PATCH_RING);
    PatchSlot &p = ix->patch[k];
    if (p.seq) {   // the slot's patch must have reached every replica and left its pinned buffer
        for (int r = 0; r < ix->nrep; r++) {
            Replica &R = ix->rep[r];
            if (R.applied < p.seq && (rc = bring_up(ix, r, p.seq, R.ps))) return rc;
            if (R.ppending[k]) {
                HIPCHK(ix, hipSetDevice(R.device));
                HIPCHK(ix, hipEventSynchronize(R.pdone[k]));
                R.ppending[k] = false;
            }
        }
    }
    const uint64_t t2 = g_col_timing ? col_now() : 0;
    const uint64_t bytes = nr * sizeof(PatchRun) + nw * 4;
    if (bytes > p.pin_cap || !p.pin) {
        if (p.pin) HIPCHK(ix, hipHostFree(p.pin));
        p.pin = nullptr;
        p.pin_cap = 0;
        const uint64_t want = std::max<uint64_t>(bytes * 2, 64u << 10);
        uint8_t *np = nullptr;   // the capacity is recorded only once the buffer exists
        HIPCHK(ix, hipHostMalloc(&np, want, hipHostMallocPortable | hipHostMallocMapped));
        p.pin = np;
        p.pin_cap = want;
        void *dp = nullptr;
        p.pin_dev = hipHostGetDevicePointer(&dp, np, 0) == hipSuccess ? static_cast<uint8_t *>(dp) : nullptr;
    }
    memcpy(p.pin, runs.data(), nr * sizeof(PatchRun));
    memcpy(p.pin + nr * sizeof(PatchRun), data.data(), nw * 4);
    p.bytes = bytes; p.nr = nr; p.seq = q;
    if (g_col_timing) {
        g_col_n++;
        g_col_runs_ns += t1 - t0; g_col_slot_ns += t2 - t1; g_col_copy_ns += col_now() - t2;
    }
    ix->patch_seq = q;
    ix->patch_bytes += nw * 4;
    ix->uploads++;
    return TM_OK;
}

// Every delta applied so far, onto replica r0 before a batch runs there on
// stream s (caller holds ix->mu; the calling thread's device is r0's after)
int sync_locked(tm_index *ix, int r0, hipStream_t s) {
    int rc;
    if ((rc = collect_patch(ix))) return rc;
    if ((rc = bring_up(ix, r0, ix->pub_seq, s))) return rc;
    HIPCHK(ix, hipSetDevice(ix->rep[r0].device));
    return TM_OK;
}

// Which copy of group g a batch should read (caller holds ix->mu, pending
// deltas collected): the lowest-numbered copy that is up to date (so without
// churn one copy stays hot), else one no batch is reading (it takes the
// patch without waiting), else the least recently used one.  busy (host
// lanes per replica) excludes copies whose host lanes are all in use.
// A device-API batch names its stream s: then a copy whose unfinished
// readers all run on s counts as idle too (the patch is ordered behind them
// by the stream itself, no cross-stream wait), preferring the copy s read
// last, so with as many copies as streams each stream keeps to its own copy
// under churn.
int pick_copy(tm_index *ix, int g, const int *busy, hipStream_t s = nullptr, bool by_stream = false) {
    auto ok = [&](int r) { return ix->rep[r].group == g && (!busy || busy[r] < MAX_HOST_LANES); };
    const int sv = ix->serving[g];   // the copy tm_commit last published on: fresh, its readers' hot set
    if (sv >= 0 && ok(sv) && ix->rep[sv].applied >= ix->pub_seq) return sv;
    for (int r = 0; r < ix->nrep; r++)
        if (ok(r) && ix->rep[r].applied >= ix->pub_seq) return r;
    if (by_stream) {
        int pick = -1;
        uint64_t pick_tick = 0;
        for (int r = 0; r < ix->nrep; r++) {
            if (!ok(r)) continue;
            bool free_here = true;
            uint64_t mine = 0;   // when stream s last read copy r (0: never)
            for (auto &l : ix->lanes) {
                if (l->r != r || !l->used) continue;
                if (l->s == s) { mine = std::max<uint64_t>(mine, l->tick); continue; }
                if (lane_busy(*l)) { free_here = false; break; }
            }
            if (free_here && (pick < 0 || mine > pick_tick)) { pick = r; pick_tick = mine; }
        }
        if (pick >= 0) return pick;
    }
    for (int r = 0; r < ix->nrep; r++) {
        if (!ok(r)) continue;
        bool idle = true;
        for (auto &l : ix->lanes)
            if (l->r == r && lane_busy(*l)) { idle = false; break; }
        if (idle) return r;
    }
    int best = -1;
    for (int r = 0; r < ix->nrep; r++)
        if (ok(r) && (best < 0 || ix->rep[r].last_use < ix->rep[best].last_use)) best = r;
    return best;
}

// the device view of replica r as of the last collect_patch (caller holds ix->mu)
DevIndex dev_view(tm_index *ix, int r) { return ix->view[r]; }

// (caller holds ix->img)
DevIndex dev_view_build(tm_index *ix, int r) {
    DevIndex d;
    d.vocab = ix->vocab.d[r]; d.vmask = (uint32_t)ix->vocab.h.size() - 1;
    d.wpool = ix->wpool.d[r];
    d.nodes = ix->nodes.d[r];
    d.ctab = ix->ctab.d[r];
    d.vals = ix->vals.d[r];
    d.exact = ix->exact.d[r]; d.xmask = (uint32_t)ix->exact.h.size() - 1;
    d.xfp = ix->xfp.d[r];
    d.wseq = ix->wseq.d[r];
    d.wbits = ix->wbits.d[r]; d.wcap = ix->wide.empty() ? 0 : ix->wb_words * 32;
    // levels a walk must resolve: the deepest live node's depth (no node below
    // it has children), all of a topic's levels when a binary key has its length
    auto &dc = ix->depth_cnt, &xc = ix->xlen_cnt;
    while (dc.size() > 1 && dc.back() == 0) dc.pop_back();
    while (!xc.empty() && xc.back() == 0) xc.pop_back();
    d.depth = dc.empty() ? 0 : (uint32_t)dc.size() - 1;
    d.xlen_max = xc.empty() ? 0 : (uint32_t)xc.size() - 1;
    d.xlen_mask = 0;
    for (size_t k = 0; k < xc.size() && k < 64; k++) if (xc[k]) d.xlen_mask |= 1ull << k;
    d.hdesc = ix->n_hdesc_keys != 0;
    for (uint32_t s = 0; s < ANX_SLOTS; s++) d.anx_depth[s] = ix->anx[s] == NONE ? NONE : ix->aux[ix->anx[s]].depth;
    return d;
}

// ------------------------------------------------------------------ lanes

void free_workspace(Workspace &w) {
    void *wb[] = {w.cnt, w.nr, w.rng, w.lists, w.list_n, w.blk, w.deep_wid, w.deep_stk, w.deep_plus, w.look, w.pairs,
                  w.vres};
    for (void *p : wb) if (p) (void)hipFree(p);
    if (w.hint_h) (void)hipHostFree(w.hint_h);
    w = Workspace{};
}

void free_lane(Lane &l) {
    free_workspace(l.w);
    void *dv[] = {l.d_in, l.d_res, l.d_vals, l.d_o64, l.d_h64, l.f.tab, l.f.tot, l.f.t, l.f.v, l.f.b, l.f.voff, l.f.sums, l.f.b2,
                  l.d_ft, l.d_fv, l.d_fo, l.d_pr, l.f.ag_bits, l.f.ag_pre, l.f.ag_cnt, l.d_at, l.d_av, l.d_ao, l.fo1_s,
                  l.f.dp_cnt, l.f.dp_off, l.f.dp_tot, l.d_dt, l.d_dv, l.d_ds, l.f.sh_key, l.f.sh_cnt, l.d_sm, l.d_sk,
                  l.f.gs_fix, l.f.gs_k[0], l.f.gp_fix, l.d_gt, l.d_gv, l.d_gs, l.d_gsub, l.d_goff};
    for (void *p : dv) if (p) (void)hipFree(p);
    void *pins[] = {l.pin_in, l.pin_out, l.pin_vals, l.fo1_h};
    for (void *p : pins) if (p) (void)hipHostFree(p);
    if (l.done) (void)hipEventDestroy(l.done);
    if (l.owned && l.s) (void)hipStreamDestroy(l.s);
}

// a lane of replica r (the calling thread's device is r's)
int make_lane(tm_index *ix, int r, hipStream_t s, bool owned, Lane *&out) {
    auto l = std::make_unique<Lane>();
    l->r = r;
    l->owned = owned;
    if (owned) HIPCHK(ix, hipStreamCreateWithFlags(&l->s, hipStreamNonBlocking));
    else l->s = s;
    HIPCHK(ix, hipEventCreateWithFlags(&l->done, hipEventDisableTiming));
    out = l.get();
    ix->lanes.push_back(std::move(l));
    return TM_OK;
}

// A host-API lane for this caller: on the group (one entry of the device
// list) with the fewest batches in flight (round robin among equals), on the
// copy pick_copy chooses there; waiting while every copy has MAX_HOST_LANES in
// use.  Pending deltas are collected first (pick_copy must know which copies
// are up to date).  Leaves the calling thread on the lane's device.
int host_lane(tm_index *ix, std::unique_lock<std::mutex> &g, Lane *&out) {
    for (;;) {
        if (int rc = collect_patch(ix)) return rc;
        int busy[MAX_REPLICAS] = {}, gbusy[MAX_REPLICAS] = {};
        bool gfree[MAX_REPLICAS] = {};
        for (auto &l : ix->lanes)
            if (l->owned) busy[l->r] += l->busy;
        for (int r = 0; r < ix->nrep; r++) {
            gbusy[ix->rep[r].group] += busy[r];
            gfree[ix->rep[r].group] |= busy[r] < MAX_HOST_LANES;
        }
        int bg = -1;
        for (int k = 0; k < ix->ngroups; k++) {
            const int gi = (int)((ix->rr + k) % ix->ngroups);
            if (gfree[gi] && (bg < 0 || gbusy[gi] < gbusy[bg])) bg = gi;
        }
        if (bg >= 0) {
            ix->rr++;
            const int best = pick_copy(ix, bg, busy);
            ix->rep[best].last_use = ++ix->tick;
            HIPCHK(ix, hipSetDevice(ix->rep[best].device));
            for (auto &l : ix->lanes)
                if (l->owned && l->r == best && !l->busy) { l->busy = true; out = l.get(); return TM_OK; }
            int rc = make_lane(ix, best, nullptr, true, out);
            if (rc) return rc;
            out->busy = true;
            return TM_OK;
        }
        ix->cv.wait(g);
    }
}

// the group of the calling thread's current HIP device (the first entry of
// the device list on it)
int dev_group(tm_index *ix, int &g) {
    int dev = 0;
    HIPCHK(ix, hipGetDevice(&dev));
    for (int r = 0; r < ix->nrep; r++)
        if (ix->rep[r].device == dev) { g = ix->rep[r].group; return TM_OK; }
    return fail(ix, TM_EINVAL, "device API: the current HIP device holds no replica of this index");
}

// the device-API lane of stream s on replica r; the least recently used one is
// retired (after its batches finish) when MAX_DEV_LANES (stream, replica)
// pairs hold a workspace
int dev_lane(tm_index *ix, hipStream_t s, int r, Lane *&out) {
    int n = 0;
    size_t lru = SIZE_MAX;
    for (size_t i = 0; i < ix->lanes.size(); i++) {
        Lane &l = *ix->lanes[i];
        if (l.owned) continue;
        if (l.s == s && l.r == r) { l.tick = ++ix->tick; out = &l; return TM_OK; }
        n++;
        if (lru == SIZE_MAX || l.tick < ix->lanes[lru]->tick) lru = i;
    }
    if (n >= MAX_DEV_LANES && lru != SIZE_MAX) {
        Lane &l = *ix->lanes[lru];
        HIPCHK(ix, hipSetDevice(ix->rep[l.r].device));
        if (l.used) HIPCHK(ix, hipEventSynchronize(l.done));
        free_lane(l);
        ix->lanes.erase(ix->lanes.begin() + lru);
    }
    HIPCHK(ix, hipSetDevice(ix->rep[r].device));
    int rc = make_lane(ix, r, s, false, out);
    if (rc) return rc;
    out->tick = ++ix->tick;
    return TM_OK;
}

template <class T>
int grow_dev(tm_index *ix, hipStream_t s, T *&p, uint64_t &cap, uint64_t need) {
    if (need <= cap && p) return TM_OK;
    HIPCHK(ix, hipStreamSynchronize(s));   // only this lane's stream uses its buffers
    if (p) HIPCHK(ix, hipFree(p));
    p = nullptr;
    cap = std::max<uint64_t>(need + need / 4, 64);
    HIPCHK(ix, hipMalloc(&p, cap * sizeof(T)));
    return TM_OK;
}

int ensure_ws(tm_index *ix, uint64_t n, Lane &ln) {
    Workspace &w = ln.w;
    if (!w.deep_wid) {
        HIPCHK(ix, hipMalloc(&w.deep_wid, (uint64_t)DEEP_LANES * MAX_LEVELS * 4));
        HIPCHK(ix, hipMalloc(&w.deep_stk, (uint64_t)DEEP_LANES * (MAX_LEVELS + 1) * 8));
        HIPCHK(ix, hipMalloc(&w.deep_plus, (uint64_t)DEEP_LANES * MAX_LEVELS));
        HIPCHK(ix, hipMalloc(&w.list_n, LIST_SLOTS * 4));
        HIPCHK(ix, hipMemsetAsync(w.list_n, 0, LIST_SLOTS * 4, ln.s));
        HIPCHK(ix, hipMalloc(&w.pairs, 2 * SMALL_SEGS * 4));
        HIPCHK(ix, hipMemsetAsync(w.pairs, 0, 2 * SMALL_SEGS * 4, ln.s));
        HIPCHK(ix, hipMalloc(&w.vres, VRES_WORDS * 8));
        HIPCHK(ix, hipMemsetAsync(w.vres, 0, VRES_WORDS * 8, ln.s));
        HIPCHK(ix, hipHostMalloc(&w.hint_h, HINT_WORDS * 4, hipHostMallocMapped));
        std::memset(w.hint_h, 0, HINT_WORDS * 4);
        HIPCHK(ix, hipHostGetDevicePointer(reinterpret_cast<void **>(&w.hint_d), w.hint_h, 0));
    }
    // the batch must see every patch shipped so far, whichever stream it went
    // on (once per patch: later batches on the lane's stream are behind it)
    if (ix->rep[ln.r].last_patch && ln.waited != ix->rep[ln.r].applied) {
        HIPCHK(ix, hipStreamWaitEvent(ln.s, ix->rep[ln.r].last_patch, 0));
        ln.waited = ix->rep[ln.r].applied;
    }
    if (n <= w.cap_n && w.cnt) return TM_OK;
    HIPCHK(ix, hipStreamSynchronize(ln.s));
    if (w.cnt) {
        void *old[] = {w.cnt, w.nr, w.rng, w.lists, w.blk, w.look};
        for (void *p : old) (void)hipFree(p);
    }
    uint64_t c = std::max<uint64_t>(n + n / 4, 1024);
    HIPCHK(ix, hipMalloc(&w.cnt, c * 4));
    HIPCHK(ix, hipMalloc(&w.nr, c * 4));
    HIPCHK(ix, hipMalloc(&w.rng, c * RCAP * 8));
    HIPCHK(ix, hipMalloc(&w.lists, c * (L_COUNT + 1) * 4));
    const uint64_t nblk = c / TILE + 4, nsup = c / ((uint64_t)TILE * SUP) + 4;
    HIPCHK(ix, hipMalloc(&w.blk, (nblk + nsup) * 8));
    HIPCHK(ix, hipMemsetAsync(w.blk, 0, (nblk + nsup) * 8, ln.s));   // zero between batches (k_rewalk_tail)
    w.sup = w.blk + nblk;
    HIPCHK(ix, hipMalloc(&w.look, (c / SM_TOPICS + 4) * 8 * LB_STRIDE));
    HIPCHK(ix, hipMemsetAsync(w.look, 0, (c / SM_TOPICS + 4) * 8 * LB_STRIDE, ln.s));   // no launch tag is 0
    w.cap_n = c;
    return TM_OK;
}

void init_tables(tm_index *ix, uint64_t hint) {
    // tables start small and double at load 1/2: their size follows the live
    // key set, so hot entries stay dense (vocab / top trie levels in L2)
    ix->vocab.h.assign(1024, empty_vocab());
    ix->exact.h.assign(1024, empty_exact());
    ix->xfp.h.assign(1024, 0);
    ix->xcap.assign(ix->exact.h.size(), 0);
    ix->xroff.assign(ix->exact.h.size(), 0);
    ix->nodes.h.reserve(hint / 2 + 1);
    ix->aux.reserve(hint / 2 + 1);
    node_new(ix, NONE, NONE, false);   // ROOT
    ix->vals.h.reserve(hint + 16);
    // a 16-B guard before the first run: k_emit's run-by-run copy loads whole
    // quads that may overhang a run by up to 3 words on either side (the
    // guard after the last run is the device copy's DEV_GUARD slack)
    ix->vals.h.assign(4, 0);
}

// NULL is HIP's default (null) stream -- the stream PyTorch's default stream
// handle (0) names, so device-API batches order with the caller's torch work
hipStream_t pick_stream(tm_index *, void *s) { return reinterpret_cast<hipStream_t>(s); }

// events of one profiled batch (null set when profiling is off)
int prof_begin(tm_index *ix, tm_index::ProfEv &ev, hipStream_t s) {
    ev = {nullptr, nullptr, nullptr, nullptr, 0};
    if (!ix->prof) return TM_OK;
    int dev = 0;
    HIPCHK(ix, hipGetDevice(&dev));
    for (size_t i = 0; i < ix->prof_free.size(); i++)   // events of this device
        if (ix->prof_free[i].device == dev) {
            ev = ix->prof_free[i];
            ix->prof_free.erase(ix->prof_free.begin() + i);
            break;
        }
    if (!ev.b0) {
        HIPCHK(ix, hipEventCreate(&ev.b0)); HIPCHK(ix, hipEventCreate(&ev.w0));
        HIPCHK(ix, hipEventCreate(&ev.w1)); HIPCHK(ix, hipEventCreate(&ev.b1));
        ev.device = dev;
    }
    HIPCHK(ix, hipEventRecord(ev.b0, s));
    return TM_OK;
}

int prof_end(tm_index *ix, tm_index::ProfEv &ev, hipStream_t s) {
    if (!ev.b0) return TM_OK;
    HIPCHK(ix, hipEventRecord(ev.b1, s));
    ix->prof_pending.push_back(ev);
    return TM_OK;
}

// wait for every batch of every lane (caller holds ix->mu)
int drain_lanes(tm_index *ix) {
    for (auto &l : ix->lanes)
        if (l->used) {
            HIPCHK(ix, hipSetDevice(ix->rep[l->r].device));
            HIPCHK(ix, hipEventSynchronize(l->done));
        }
    return TM_OK;
}

// the lane a fan-out on stream s uses: the one the stream's match batches use, if any
int fanout_lane(tm_index *ix, hipStream_t s, int grp, Lane *&ln) {
    for (auto &l : ix->lanes)
        if (!l->owned && l->s == s && ix->rep[l->r].group == grp) { ln = l.get(); ln->tick = ++ix->tick; return TM_OK; }
    int r = 0;
    while (ix->rep[r].group != grp) r++;
    return dev_lane(ix, s, r, ln);
}

// TM_HOST_TIMING=1 (diagnostics): host timings on stderr, per tm_match_batch and summed by tm_destroy
static const bool g_cmb_timing = getenv("TM_HOST_TIMING") != nullptr;
static inline uint64_t ns_now() {
    return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(
        std::chrono::steady_clock::now().time_since_epoch()).count();
}

// A device-API call: it holds the index lock throughout (nothing waits for
// the GPU) and queues on the caller's stream, on the group of the calling
// thread's device.  An entry point checks its arguments, opens one of the two
// kinds, queues its kernels on `s` and returns done().
struct DevBatch {
    tm_index *ix;
    std::lock_guard<std::mutex> g;
    hipStream_t s;
    int grp = 0;
    Lane *ln = nullptr;
    DevIndex d;   // (open_match) the copy's view
    tm_index::ProfEv ev{nullptr, nullptr, nullptr, nullptr, 0};
    DevBatch(tm_index *ix, void *stream) : ix(ix), g(ix->mu), s(pick_stream(ix, stream)) {}
    // a match batch of n topics: pending deltas collected, the copy picked and
    // counted, its lane on `s` brought up to date with a workspace for n
    int open_match(uint64_t n) {
        int rc;
        if ((rc = dev_group(ix, grp))) return rc;
        if ((rc = collect_patch(ix))) return rc;
        const int r = pick_copy(ix, grp, nullptr, s, true);
        ix->rep[r].last_use = ++ix->tick;
        ix->rep[r].batches++;
        if ((rc = dev_lane(ix, s, r, ln))) return rc;
        if ((rc = sync_locked(ix, ln->r, s))) return rc;
        if ((rc = ensure_ws(ix, n, *ln))) return rc;
        d = dev_view(ix, ln->r);
        return prof_begin(ix, ev, s);
    }
    // a fan-out or aggre pass over the caller's device arrays: only the lane (its scratch)
    int open_fanout() {
        if (int rc = dev_group(ix, grp)) return rc;
        return fanout_lane(ix, s, grp, ln);
    }
    int done() {
        if (int rc = batch_done(ix, *ln)) return rc;
        return prof_end(ix, ev, s);
    }
};

// A host-API batch: the index lock, the lane checked out for the call, the
// workspace it asked for and the call's retry count.  Host-API batches hold
// the lock only to ship pending patches, pick up the index's current device
// view and queue the kernels on their lane; they wait for the GPU and copy
// results out without it, so concurrent callers overlap on the device (each
// lane is its own stream) and deltas keep flowing.  An entry point checks its
// arguments, open()s, and gives run() what it queues; relock() is the only way
// back under the lock after run() dropped it (a retry, a scratch that grew).
// The lane is released on every exit path, under the lock (retaken if need
// be).  Round 6 measured releasing it without the lock (an atomic flag,
// waiters announced): the leader's 55-85 us wait for the lock after its GPU
// wait went, and 16 concurrent callers lost 10-15 % (4.0-4.1 vs 4.8-4.9e8
// topics/s, profiles/r6/lane_release/) -- the lock paces the leaders; kept.
struct HostBatch {
    tm_index *ix;
    std::unique_lock<std::mutex> g;
    Lane *ln = nullptr;
    uint64_t ws_topics = 0;
    int tries = 0;
    uint64_t t_queued = 0, t_synced = 0;   // (TM_HOST_TIMING) the last attempt: lock dropped, GPU wait over
    const char *who;   // the entry point, for the messages
    explicit HostBatch(tm_index *ix, const char *who = "tm_match_batch") : ix(ix), g(ix->mu), who(who) {}
    ~HostBatch() {
        if (!ln) return;
        if (!g.owns_lock()) g.lock();
        ln->busy = false;
        ix->cv.notify_one();
    }
    // a lane, up to date, with a workspace for ws topics (the batch is counted
    // by the caller, once it is known to run here)
    int open(uint64_t ws) {
        int rc;
        ws_topics = ws;
        if ((rc = host_lane(ix, g, ln))) return rc;
        if ((rc = sync_locked(ix, ln->r, ln->s))) return rc;
        return ensure_ws(ix, ws_topics, *ln);
    }
    // ensure_ws too: while the lock was away another caller may have patched
    // this copy on its own stream, and that is where the lane's stream waits
    // for the copy's last patch
    int relock() {
        g.lock();
        HIPCHK(ix, hipSetDevice(ix->rep[ln->r].device));
        if (int rc = sync_locked(ix, ln->r, ln->s)) return rc;
        return ensure_ws(ix, ws_topics, *ln);
    }
    // queue(view, tag) queues the batch on ln->s (and counts its path); then
    // the lock is dropped for the GPU wait.  A failed one-launch batch (its
    // look-back wait expired: err 4 flags, never a client error -- the
    // reference raises badarg only for a '+'/'#' level,
    // emqx_trie_search.erl:374-375) runs again, on the same lane with the
    // current device view, once per call; the second failure is TM_EDEVICE
    // for the whole call.
    template <class Queue>
    int run(Queue &&queue) {
        for (;;) {
            int rc;
            uint32_t tag;
            if ((rc = next_tag(ix, *ln, ln->s, tag))) return rc;
            if ((rc = queue(dev_view(ix, ln->r), tag))) return rc;
            if ((rc = batch_done(ix, *ln))) return rc;
            g.unlock();
            if (g_cmb_timing) t_queued = ns_now();
            HIPCHK(ix, hipStreamSynchronize(ln->s));
            if (g_cmb_timing) t_synced = ns_now();
            if (!batch_failed(ix, *ln)) return TM_OK;
            if (tries++ >= 1)
                return fail(ix, TM_EDEVICE, std::string(who) + ": the batch failed on the device twice (look-back wait "
                                                               "expired, err 4); not matched");
            ix->retried_batches++;
            if ((rc = relock())) return rc;
        }
    }
};

}  // namespace

// =================================================================== C ABI

extern "C" {

uint32_t tm_abi_version(void) { return (1u << 16) | 25u; }

const char *tm_last_error(tm_index *) { return g_last_error.c_str(); }

int tm_create_replicas(const tm_options *opts, const int32_t *devices, uint32_t n, tm_index **out) {
    if (!out) return fail(nullptr, TM_EINVAL, "tm_create: out is NULL");
    *out = nullptr;
    const uint32_t copies = opts && opts->copies ? opts->copies : 1;
    if (!devices || n == 0 || n > 8 || copies > 4 || n * copies > (uint32_t)MAX_REPLICAS)
        return fail(nullptr, TM_EINVAL, "tm_create_replicas: 1 to 8 devices, 1 to 4 copies, at most 16 replicas");
    tm_index *ix = new (std::nothrow) tm_index();
    if (!ix) return fail(nullptr, TM_ENOMEM, "tm_create: out of host memory");
    ix->nrep = (int)(n * copies);
    for (int g = 0; g < MAX_REPLICAS; g++) ix->serving[g] = -1;
    ix->ngroups = (int)n;
    hipError_t e = hipSuccess;
    for (uint32_t r = 0; r < n * copies && e == hipSuccess; r++) {
        Replica &R = ix->rep[r];
        R.device = devices[r / copies];
        R.group = (int)(r / copies);
        e = hipSetDevice(R.device);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&R.ps, hipStreamNonBlocking);
        for (int i = 0; i < PATCH_RING && e == hipSuccess; i++)
            e = hipEventCreateWithFlags(&R.pdone[i], hipEventDisableTiming);
    }
    if (e != hipSuccess) {
        std::string m = std::string("tm_create: ") + hipGetErrorString(e);
        tm_destroy(ix);
        return fail(nullptr, TM_EDEVICE, m);
    }
    (void)hipSetDevice(ix->rep[0].device);
    init_tables(ix, opts ? opts->hint_keys : 0);
    *out = ix;
    return TM_OK;
}

int tm_create(const tm_options *opts, tm_index **out) {
    int32_t dev = opts ? opts->device : -1;
    if (dev < 0) {
        int d = 0;
        if (hipGetDevice(&d) != hipSuccess) d = 0;
        dev = d;
    }
    return tm_create_replicas(opts, &dev, 1, out);
}

int tm_replica_stats(tm_index *ix, uint32_t r, uint64_t *batches, int32_t *device) {
    if (!ix) return fail(nullptr, TM_EINVAL, "tm_replica_stats: null handle");
    std::lock_guard<std::mutex> g(ix->mu);
    if (r >= (uint32_t)ix->nrep) return fail(ix, TM_EINVAL, "tm_replica_stats: no such replica");
    if (batches) *batches = ix->rep[r].batches;
    if (device) *device = ix->rep[r].device;
    return TM_OK;
}

namespace { void mf_free_keys(tm_index::MfState &m); }

// TM_HOST_TIMING=1 (diagnostics): where a combined launch's host time goes,
// summed over the process and printed by tm_destroy
struct CmbTiming {
    std::atomic<uint64_t> groups{0}, reqs{0};
    std::atomic<uint64_t> lock_ns{0}, setup_ns{0}, launch_ns{0}, sync_ns{0}, release_ns{0}, done_ns{0}, req_ns{0};
};
static CmbTiming g_cmbt;
// (TM_HOST_TIMING) where tm_commit's time goes
struct CommitTiming {
    std::atomic<uint64_t> n{0}, apply_ns{0}, lock_ns{0}, collect_ns{0}, idle_ns{0}, ship_ns{0};
};
static CommitTiming g_cmt;

int tm_destroy(tm_index *ix) {
    if (!ix) return TM_EINVAL;
    if (g_cmb_timing && g_cmbt.groups) {
        const double g = (double)g_cmbt.groups, us = 1e-3;
        fprintf(stderr, "tm combiner: %lu launches, %lu requests (%.2f per launch); per launch us: lock %.1f "
                        "setup %.1f launch %.1f sync %.1f lane-release %.1f mark-done %.1f; per request %.1f us\n",
                (unsigned long)g_cmbt.groups.load(), (unsigned long)g_cmbt.reqs.load(), g_cmbt.reqs / g,
                g_cmbt.lock_ns * us / g, g_cmbt.setup_ns * us / g, g_cmbt.launch_ns * us / g, g_cmbt.sync_ns * us / g,
                g_cmbt.release_ns * us / g, g_cmbt.done_ns * us / g,
                g_cmbt.req_ns * us / std::max<double>(1.0, (double)g_cmbt.reqs));
    }
    if (g_cmb_timing && g_col_n) {
        const double c = (double)g_col_n, us = 1e-3;
        fprintf(stderr, "tm collect: %lu patches; per patch us: runs %.1f slot-reuse %.1f pinned-copy %.1f\n",
                (unsigned long)g_col_n.load(), g_col_runs_ns * us / c, g_col_slot_ns * us / c, g_col_copy_ns * us / c);
    }
    if (g_cmb_timing && g_cmt.n) {
        const double c = (double)g_cmt.n, us = 1e-3;
        fprintf(stderr, "tm commit: %lu commits; per commit us: image %.1f lock %.1f collect %.1f wait-idle %.1f "
                        "ship %.1f\n", (unsigned long)g_cmt.n.load(), g_cmt.apply_ns * us / c, g_cmt.lock_ns * us / c,
                g_cmt.collect_ns * us / c, g_cmt.idle_ns * us / c, g_cmt.ship_ns * us / c);
    }
    for (int r = 0; r < ix->nrep; r++) {
        (void)hipSetDevice(ix->rep[r].device);
        (void)hipDeviceSynchronize();
    }
    for (auto &l : ix->lanes) {
        (void)hipSetDevice(ix->rep[l->r].device);
        free_lane(*l);
    }
    for (int r = 0; r < ix->nrep; r++) {
        Replica &R = ix->rep[r];
        (void)hipSetDevice(R.device);
        void *bufs[] = {ix->vocab.d[r], ix->wpool.d[r], ix->nodes.d[r], ix->ctab.d[r], ix->vals.d[r], ix->exact.d[r],
                        ix->xfp.d[r], ix->wseq.d[r], ix->wbits.d[r]};
        for (void *p : bufs) if (p) (void)hipFree(p);
        for (int i = 0; i < PATCH_RING; i++) {
            if (R.pdev[i]) (void)hipFree(R.pdev[i]);
            if (R.pdone[i]) (void)hipEventDestroy(R.pdone[i]);
        }
        if (R.ps) (void)hipStreamDestroy(R.ps);
    }
    for (int g = 0; g < ix->ngroups; g++) {
        for (int r = 0; r < ix->nrep; r++)
            if (ix->rep[r].group == g) { (void)hipSetDevice(ix->rep[r].device); break; }
        for (auto *D : {&ix->dest[g], &ix->filt[g], &ix->sub_pool[g], &ix->sub_span[g], &ix->share_slot[g],
                        &ix->share_rec[g], &ix->share_pool[g], &ix->msub[g]}) {
            if (D->d) (void)hipFree(D->d);
            if (D->pin) (void)hipHostFree(D->pin);
            if (D->ev) (void)hipEventDestroy(D->ev);
        }
        if (ix->share_state[g].d) (void)hipFree(ix->share_state[g].d);
    }
    (void)hipSetDevice(ix->rep[0].device);
    mf_free_keys(ix->mf);
    for (void *p : {(void *)ix->mf.q, (void *)ix->mf.err, (void *)ix->mf.hit, (void *)ix->mf.out}) if (p) (void)hipFree(p);
    if (ix->mf.s) (void)hipStreamDestroy(ix->mf.s);
    for (auto &p : ix->patch) if (p.pin) (void)hipHostFree(p.pin);
    for (auto &b : ix->pinned) (void)(b.vram ? hipFree(b.host) : hipHostFree(b.host));
    for (auto *v : {&ix->prof_pending, &ix->prof_free})
        for (auto &ev : *v) {
            (void)hipSetDevice(ev.device);
            for (hipEvent_t x : {ev.b0, ev.w0, ev.w1, ev.b1}) (void)hipEventDestroy(x);
        }
    delete ix;
    return TM_OK;
}

int tm_apply_deltas_ex(tm_index *ix, uint64_t n, const uint8_t *ops, const uint8_t *fb, const uint64_t *fo,
                       const uint32_t *values, const uint8_t *key_flags, uint64_t *out_epoch) {
    if (!ix) return fail(nullptr, TM_EINVAL, "tm_apply_deltas: null handle");
    if (n && (!ops || !fo || !values || (!fb && fo[n] != fo[0])))
        return fail(ix, TM_EINVAL, "tm_apply_deltas: null buffer");
    for (uint64_t i = 0; i < n; i++)
        if (ops[i] > TM_OP_INSERT || fo[i + 1] < fo[i] || fo[i + 1] - fo[i] > 0xFFFFFFFFull)
            return fail(ix, TM_EINVAL, "tm_apply_deltas: bad op or offsets at " + std::to_string(i));
    std::lock_guard<std::mutex> g(ix->img);   // the host image only: batches without a delta to pick up go on
    std::vector<WordRef> w;
    std::vector<uint32_t> wids;
    try {
        for (uint64_t i = 0; i < n; i++)
            key_op(ix, ops[i] == TM_OP_INSERT, fb + fo[i], (uint32_t)(fo[i + 1] - fo[i]), values[i],
                   key_flags ? key_flags[i] : 0, w, wids);
        reclaim(ix);
        wide_dense(ix);
        annex_designate(ix);
    } catch (const std::bad_alloc &) {
        return fail(ix, TM_ENOMEM, "tm_apply_deltas: out of host memory");
    }
    // the keys changed above are what every batch queued from now on sees:
    // a reader registered from now on begins at the new epoch
    if (n) ix->img_dirty.store(true, std::memory_order_release);
    const uint64_t e = n ? ix->epoch.fetch_add(1, std::memory_order_acq_rel) + 1 : ix->epoch.load();
    if (out_epoch) *out_epoch = e;
    return TM_OK;
}

int tm_apply_deltas(tm_index *ix, uint64_t n, const uint8_t *ops, const uint8_t *fb, const uint64_t *fo,
                    const uint32_t *values, const uint8_t *key_flags) {
    return tm_apply_deltas_ex(ix, n, ops, fb, fo, values, key_flags, nullptr);
}

// tm_commit (include/tmatch.h): the deltas reach the host image while
// batches are held off collecting them (img_hold), then -- under the device
// lock -- one patch is collected and applied to a copy of each group that no
// batch is reading, which becomes the group's serving copy, and only then is
// the patch published (pub_seq): batches queued afterwards read that copy,
// and no batch ever waits on the GPU for this patch.  While every copy of a
// group has readers the committer waits (the lock released) for one to
// drain, up to COMMIT_WAIT; past it -- or with one copy per group -- the
// patch is published as tm_apply_deltas' are (batches take it in stream
// order, behind the batches reading that copy).
// The collect also refreshes every copy's cached view and may ship whole
// tables to all of them, while a batch queued during that wait skips its own
// collect (img_hold) and brings its copy up to the old pub_seq only: it would
// walk with the new view (a smaller depth, a cleared xlen_mask bit, new table
// pointers) over tables that lack the patch.  So a commit whose collect
// changed a view or shipped a table whole never waits: it publishes before
// the lock is released, as if past COMMIT_WAIT.
constexpr auto COMMIT_WAIT = std::chrono::milliseconds(20);

// what a launch reads of a copy's cached view, field by field (the struct has
// padding); a field added to DevIndex belongs here too, or a change of it alone
// would let a commit wait again
static_assert(sizeof(DevIndex) == 128, "DevIndex changed: compare the new field in same_view");
static bool same_view(const DevIndex &a, const DevIndex &b) {
    return a.vocab == b.vocab && a.vmask == b.vmask && a.wpool == b.wpool && a.nodes == b.nodes && a.ctab == b.ctab &&
           a.vals == b.vals && a.exact == b.exact && a.xmask == b.xmask && a.xfp == b.xfp && a.wseq == b.wseq &&
           a.wbits == b.wbits && a.wcap == b.wcap && a.depth == b.depth && a.xlen_max == b.xlen_max &&
           a.xlen_mask == b.xlen_mask && a.hdesc == b.hdesc && a.anx_depth[0] == b.anx_depth[0] &&
           a.anx_depth[1] == b.anx_depth[1];
}

int tm_commit(tm_index *ix, uint64_t n, const uint8_t *ops, const uint8_t *fb, const uint64_t *fo,
              const uint32_t *values, const uint8_t *key_flags, uint64_t *out_epoch) {
    if (!ix) return fail(nullptr, TM_EINVAL, "tm_commit: null handle");
    ix->img_hold.fetch_add(1, std::memory_order_acq_rel);
    struct Unhold {
        tm_index *ix;
        ~Unhold() { ix->img_hold.fetch_sub(1, std::memory_order_acq_rel); }
    } unhold{ix};
    const uint64_t ta = g_cmb_timing ? ns_now() : 0;
    int rc = tm_apply_deltas_ex(ix, n, ops, fb, fo, values, key_flags, out_epoch);
    if (rc || !n) return rc;
    const uint64_t tb = g_cmb_timing ? ns_now() : 0;
    std::unique_lock<std::mutex> g(ix->mu);
    const uint64_t tc = g_cmb_timing ? ns_now() : 0;
    const bool had_view = ix->view_ok;
    const uint64_t uploads0 = ix->uploads;
    DevIndex view0[MAX_REPLICAS];
    for (int r = 0; r < ix->nrep; r++) view0[r] = ix->view[r];
    if ((rc = collect_patch(ix, true))) return rc;
    const uint64_t q = ix->patch_seq;
    if (ix->pub_seq >= q) return TM_OK;   // (nothing to ship: the deltas changed no device word)
    ix->commits++;
    // more than the one patch uploaded, or a view changed: old tables cannot serve the new views (see above)
    bool no_wait = !had_view || ix->uploads - uploads0 > 1;
    for (int r = 0; r < ix->nrep && !no_wait; r++) no_wait = !same_view(view0[r], ix->view[r]);
    const uint64_t td = g_cmb_timing ? ns_now() : 0;
    uint64_t t_idle = 0, t_ship = 0;
    const auto t0 = std::chrono::steady_clock::now();
    bool done[MAX_REPLICAS] = {}, waited = false;
    int left = ix->ngroups;
    for (;;) {
        const bool late = no_wait || std::chrono::steady_clock::now() - t0 > COMMIT_WAIT;
        bool busy[MAX_REPLICAS] = {};   // copies with a batch still reading them (one event query per lane)
        for (auto &l : ix->lanes)
            if (!busy[l->r] && lane_busy(*l)) busy[l->r] = true;
        for (int gi = 0; gi < ix->ngroups; gi++) {
            if (done[gi]) continue;
            int pick = -1, copies = 0;
            for (int r = 0; r < ix->nrep; r++) {
                if (ix->rep[r].group != gi) continue;
                copies++;
                // the idle copy that lags most: every copy takes every patch in
                // turn, so none falls PATCH_RING behind (a ring slot's reuse
                // would otherwise bring a lagging copy up and wait for it
                // under the index lock)
                if (!busy[r] && (pick < 0 || ix->rep[r].applied < ix->rep[pick].applied)) pick = r;
            }
            if (pick < 0 && copies > 1 && !late) continue;   // wait for a copy to drain
            if (pick >= 0 && copies > 1) {
                const uint64_t t0s = g_cmb_timing ? ns_now() : 0;
                if ((rc = bring_up(ix, pick, q, ix->rep[pick].ps, true))) return rc;
                if (g_cmb_timing) t_ship += ns_now() - t0s;
                ix->serving[gi] = pick;
            } else {
                ix->commit_forced++;   // published below; the group's batches take the patch themselves
            }
            done[gi] = true;
            left--;
        }
        if (!left) break;
        waited = true;
        const uint64_t tw = g_cmb_timing ? ns_now() : 0;
        g.unlock();
        std::this_thread::sleep_for(std::chrono::microseconds(2));
        g.lock();
        if (g_cmb_timing) t_idle += ns_now() - tw;
    }
    if (waited) ix->commit_waits++;
    if (ix->pub_seq < q) ix->pub_seq = q;
    if (g_cmb_timing) {
        g_cmt.n++;
        g_cmt.apply_ns += tb - ta; g_cmt.lock_ns += tc - tb; g_cmt.collect_ns += td - tc;
        g_cmt.idle_ns += t_idle; g_cmt.ship_ns += t_ship;
    }
    return TM_OK;
}

int tm_read_begin(tm_index *ix, uint64_t *ticket) {
    if (!ix || !ticket) return fail(ix, TM_EINVAL, "tm_read_begin: null argument");
    std::lock_guard<std::mutex> g(ix->ep_mu);
    const uint64_t e = ix->epoch.load(std::memory_order_acquire);
    *ticket = ix->next_ticket++;
    ix->readers.emplace(*ticket, e);
    ix->reader_epochs.insert(e);
    return TM_OK;
}

int tm_read_end(tm_index *ix, uint64_t ticket) {
    if (!ix) return fail(nullptr, TM_EINVAL, "tm_read_end: null handle");
    std::lock_guard<std::mutex> g(ix->ep_mu);
    auto it = ix->readers.find(ticket);
    if (it == ix->readers.end()) return fail(ix, TM_EINVAL, "tm_read_end: unknown ticket");
    ix->reader_epochs.erase(ix->reader_epochs.find(it->second));
    ix->readers.erase(it);
    return TM_OK;
}

int tm_epoch(tm_index *ix, uint64_t *current, uint64_t *safe) {
    if (!ix) return fail(nullptr, TM_EINVAL, "tm_epoch: null handle");
    std::lock_guard<std::mutex> g(ix->ep_mu);
    const uint64_t e = ix->epoch.load(std::memory_order_acquire);
    if (current) *current = e;
    if (safe) *safe = ix->reader_epochs.empty() ? e : *ix->reader_epochs.begin();
    return TM_OK;
}

int tm_sync(tm_index *ix, void *stream) {
    if (!ix) return fail(nullptr, TM_EINVAL, "tm_sync: null handle");
    std::lock_guard<std::mutex> g(ix->mu);
    int dev = 0, r0 = 0;   // `stream` belongs to the current device: its replica (else replica 0, its patch stream)
    HIPCHK(ix, hipGetDevice(&dev));
    hipStream_t s = pick_stream(ix, stream);
    bool found = false;
    for (int r = 0; r < ix->nrep && !found; r++) if (ix->rep[r].device == dev) { r0 = r; found = true; }
    if (!found) s = ix->rep[0].ps;
    return sync_locked(ix, r0, s);
}

int tm_match_batch_dev_ex(tm_index *ix, uint64_t n, const uint8_t *bytes, const uint64_t *offs, uint64_t *hit_offs,
                          uint32_t *out, uint64_t cap, uint8_t *err, uint32_t order, uint32_t *ucnt, void *stream) {
    if (!ix) return fail(nullptr, TM_EINVAL, "tm_match_batch_dev: null handle");
    if (!hit_offs || (n && (!offs || !bytes || !err))) return fail(ix, TM_EINVAL, "tm_match_batch_dev: null buffer");
    if (n >= 0xFFFFFFFFull) return fail(ix, TM_EINVAL, "tm_match_batch_dev: batch too large");
    if (order > TM_ORDER_UNIQUE) return fail(ix, TM_EINVAL, "tm_match_batch_dev: bad order");
    DevBatch b(ix, stream);
    int rc;
    if ((rc = b.open_match(n))) return rc;
    uint32_t tag;
    if ((rc = next_tag(ix, *b.ln, b.s, tag))) return rc;
    // (asynchronous: a failed look-back reaches the caller as err 4 flags, include/tmatch.h)
    int path = PATH_PHASES;
    HIPCHK(ix, launch_match(b.d, b.ln->w, n, bytes, offs, hit_offs, err, out, out ? cap : 0, tag, next_lb(ix),
                            ix->dbg_phases, ix->small_kind, b.s, b.ev.w0, b.ev.w1, &path));
    ix->path_batches[path]++;
    if (order != TM_ORDER_TRAVERSAL && out)
        HIPCHK(ix, launch_sort_segments(b.ln->w, n, hit_offs, out, cap, order == TM_ORDER_UNIQUE, ucnt, b.s));
    return b.done();
}

int tm_match_batch_dev_pairs(tm_index *ix, uint64_t n, const uint8_t *bytes, const uint64_t *offs, uint32_t *pairs,
                             uint32_t *out, uint64_t cap, uint8_t *err, void *stream) {
    if (!ix) return fail(nullptr, TM_EINVAL, "tm_match_batch_dev_pairs: null handle");
    if (!pairs || (n && (!offs || !bytes || !err))) return fail(ix, TM_EINVAL, "tm_match_batch_dev_pairs: null buffer");
    if (reinterpret_cast<uintptr_t>(pairs) & 7) return fail(ix, TM_EINVAL, "tm_match_batch_dev_pairs: pairs not 8-byte aligned");
    if (n >= 0xFFFFFFFFull) return fail(ix, TM_EINVAL, "tm_match_batch_dev_pairs: batch too large");
    if (!out) cap = 0;
    if (cap > 0xFFFFFFFFull) cap = 0xFFFFFFFFull;   // (32-bit positions)
    DevBatch b(ix, stream);
    if (int rc = b.open_match(n)) return rc;
    HIPCHK(ix, launch_match_pairs(b.d, b.ln->w, n, bytes, offs, err, pairs, out, cap, b.s, b.ev.w0, b.ev.w1));
    ix->path_batches[PATH_PHASES]++;
    return b.done();
}

int tm_match_batch_dev(tm_index *ix, uint64_t n, const uint8_t *bytes, const uint64_t *offs, uint64_t *hit_offs,
                       uint32_t *out, uint64_t cap, uint8_t *err, void *stream) {
    return tm_match_batch_dev_ex(ix, n, bytes, offs, hit_offs, out, cap, err, TM_ORDER_TRAVERSAL, nullptr, stream);
}

int tm_sort_segments(tm_index *ix, uint64_t n, const uint64_t *hit_offs, uint32_t *vals, uint64_t cap, uint32_t order,
                     uint32_t *ucnt, void *stream) {
    if (!ix) return fail(nullptr, TM_EINVAL, "tm_sort_segments: null handle");
    if (!hit_offs || (cap && !vals) || order > TM_ORDER_UNIQUE) return fail(ix, TM_EINVAL, "tm_sort_segments: bad argument");
    if (n >= 0xFFFFFFFFull) return fail(ix, TM_EINVAL, "tm_sort_segments: too many segments");
    if (order == TM_ORDER_TRAVERSAL || !n) return TM_OK;
    std::lock_guard<std::mutex> g(ix->mu);
    hipStream_t s = pick_stream(ix, stream);
    Lane *ln;
    int rc, grp = 0;
    if ((rc = dev_group(ix, grp))) return rc;
    int r = 0;
    while (ix->rep[r].group != grp) r++;
    if ((rc = dev_lane(ix, s, r, ln))) return rc;
    if ((rc = ensure_ws(ix, n, *ln))) return rc;
    HIPCHK(ix, launch_sort_segments(ln->w, n, hit_offs, vals, cap, order == TM_ORDER_UNIQUE, ucnt, s));
    return batch_done(ix, *ln);
}

}  // extern "C"

namespace {

// the fan-out's scratch on a lane: the tables always, the triples of a first
// pass when n_dests needs two (grow-only; freed with the lane).  pairs (a batch
// of n topics given as spans, tm_fanout_dev_pairs): the triples for every
// n_dests, the virtual offsets and the tile sums, and a second bucket array
// when n_dests needs two passes.
int ensure_fanout(tm_index *ix, Lane &ln, uint32_t n_dests, uint64_t cap, bool pairs = false, uint64_t n = 0) {
    FanoutScratch &f = ln.f;
    if (!f.tab) {
        HIPCHK(ix, hipMalloc(&f.tab, (uint64_t)FO_BINS * FO_GRID * 4));
        HIPCHK(ix, hipMalloc(&f.tot, FO_BINS * 4));
    }
    const bool two = fanout_two_pass(n_dests);
    if (pairs) {
        if (!f.sums) HIPCHK(ix, hipMalloc(&f.sums, FP_TILES * 8));
        if (n + 1 > f.voff_cap) {
            HIPCHK(ix, hipStreamSynchronize(ln.s));
            if (f.voff) (void)hipFree(f.voff);
            f.voff = nullptr;
            f.voff_cap = 0;
            const uint64_t c = std::max<uint64_t>(n + 1 + n / 4, 1024);
            if (hipMalloc(&f.voff, c * 8) != hipSuccess) {
                (void)hipGetLastError();
                return fail(ix, TM_ENOMEM, "fan-out: no device memory for a pairs batch's offsets (8 bytes x n)");
            }
            f.voff_cap = c;
        }
    }
    if ((two || pairs) && !(cap <= f.cap && f.t)) {
        HIPCHK(ix, hipStreamSynchronize(ln.s));   // only this lane's stream uses them
        for (uint32_t **p : {&f.t, &f.v, &f.b, &f.b2}) {
            if (*p) (void)hipFree(*p);
            *p = nullptr;
        }
        f.cap = 0;
        const uint64_t c = std::max<uint64_t>(std::min<uint64_t>(cap + cap / 4, 0xFFFFFFFFull), 1024);
        for (uint32_t **p : {&f.t, &f.v, &f.b})
            if (hipMalloc(p, c * 4) != hipSuccess) {
                (void)hipGetLastError();
                return fail(ix, TM_ENOMEM, "fan-out: no device memory for the batch's scratch (12 bytes x cap)");
            }
        f.cap = c;
    }
    if (two && pairs && !f.b2 && hipMalloc(&f.b2, f.cap * 4) != hipSuccess) {
        (void)hipGetLastError();
        return fail(ix, TM_ENOMEM, "fan-out: no device memory for a two-pass pairs batch's scratch (16 bytes x cap)");
    }
    return TM_OK;
}

// The index's own value -> destination table on group g, current as of now,
// for a fan-out about to be queued on stream s (caller holds ix->mu, the
// calling thread is on the group's device).  The entries tm_set_dests changed
// since the group's last upload go up through pinned staging, in stream
// order, after the fan-outs of other streams that may still read them; a
// fan-out on another stream waits for the upload's event.
int table_upload_locked(tm_index *ix, const std::vector<uint32_t> &host, tm_index::DestDev &D, int g, hipStream_t s,
                        const uint32_t *&d, uint64_t &len) {   // (caller holds ix->dst_mu)
    const uint64_t hl = host.size();
    if (!D.ev) HIPCHK(ix, hipEventCreateWithFlags(&D.ev, hipEventDisableTiming));
    if (D.ev_set && hipEventQuery(D.ev) == hipSuccess) D.ev_set = false;
    if (hl > D.cap) {
        // grows (by half: rare): no fan-out may still read the old copy, so
        // wait for the group's lanes that have a batch in flight and for the
        // last upload -- under both locks, but not for the rest of the device
        for (auto &l : ix->lanes)
            if (ix->rep[l->r].group == g && lane_busy(*l)) HIPCHK(ix, hipEventSynchronize(l->done));
        if (D.ev_set) HIPCHK(ix, hipEventSynchronize(D.ev));
        if (D.d) HIPCHK(ix, hipFree(D.d));
        D.d = nullptr;
        D.cap = D.len = 0;
        const uint64_t c = std::max<uint64_t>(hl + hl / 2, 4096);
        HIPCHK(ix, hipMalloc(&D.d, c * 4));
        D.cap = c;
        D.lo = 0;
        D.hi = hl;
        D.ev_set = false;
    }
    if (D.hi > D.lo) {
        const uint64_t cnt = D.hi - D.lo;
        if (D.ev_set) HIPCHK(ix, hipEventSynchronize(D.ev));   // the staging buffer's last copy
        if (cnt > D.pin_cap) {
            if (D.pin) HIPCHK(ix, hipHostFree(D.pin));
            D.pin = nullptr;
            D.pin_cap = 0;
            const uint64_t c = std::max<uint64_t>(cnt + cnt / 4, 4096);
            HIPCHK(ix, hipHostMalloc(&D.pin, c * 4, hipHostMallocDefault));
            D.pin_cap = c;
        }
        std::memcpy(D.pin, host.data() + D.lo, cnt * 4);
        for (auto &l : ix->lanes)
            if (l->s != s && ix->rep[l->r].group == g && lane_busy(*l)) HIPCHK(ix, hipStreamWaitEvent(s, l->done, 0));
        HIPCHK(ix, hipMemcpyAsync(D.d + D.lo, D.pin, cnt * 4, hipMemcpyHostToDevice, s));
        HIPCHK(ix, hipEventRecord(D.ev, s));
        D.ev_set = true;
        D.ev_s = s;
        D.lo = D.hi = 0;
        D.len = hl;
    } else if (D.ev_set && D.ev_s != s) {
        HIPCHK(ix, hipStreamWaitEvent(s, D.ev, 0));
    }
    d = D.d;
    len = D.len;
    return TM_OK;
}

int table_upload(tm_index *ix, const std::vector<uint32_t> &host, tm_index::DestDev &D, int g, hipStream_t s,
                 const uint32_t *&d, uint64_t &len) {
    std::lock_guard<std::mutex> dg(ix->dst_mu);
    return table_upload_locked(ix, host, D, g, s, d, len);
}

int dest_upload(tm_index *ix, int g, hipStream_t s, const uint32_t *&d, uint64_t &len) {
    return table_upload(ix, ix->dest_h, ix->dest[g], g, s, d, len);
}

// the same for the index's value -> filter id table (tm_set_route_filters)
int filter_upload(tm_index *ix, int g, hipStream_t s, const uint32_t *&d, uint64_t &len) {
    return table_upload(ix, ix->filt_h, ix->filt[g], g, s, d, len);
}

// the index's subscriber table (tm_set_subscribers) on group g: the pool, then
// the spans, in one hold of the lock -- a tm_set_subscribers between the two
// would leave new spans over an old pool.  span_len in values.
int subs_upload(tm_index *ix, int g, hipStream_t s, const uint32_t *&span, uint64_t &span_len, const uint32_t *&pool,
                uint64_t &pool_len) {
    std::lock_guard<std::mutex> dg(ix->dst_mu);
    if (int rc = table_upload_locked(ix, ix->subs_h.pool, ix->sub_pool[g], g, s, pool, pool_len)) return rc;
    if (int rc = table_upload_locked(ix, ix->subs_h.span, ix->sub_span[g], g, s, span, span_len)) return rc;
    span_len /= 2;
    return TM_OK;
}

// the dispatch's scratch on a lane (grow-only; freed with the lane): a count
// per entry below cap, the offsets when the caller takes none, the chunk sums
int ensure_dispatch(tm_index *ix, Lane &ln, uint64_t cap, bool offsets) {
    FanoutScratch &f = ln.f;
    if (!f.dp_tot && hipMalloc(&f.dp_tot, ((uint64_t)FO_GRID + 1) * 8) != hipSuccess) {
        (void)hipGetLastError();
        f.dp_tot = nullptr;
        return fail(ix, TM_ENOMEM, "dispatch: no device memory for the pass's chunk sums (32 KiB)");
    }
    if (!(cap <= f.dp_cap && f.dp_cnt)) {
        HIPCHK(ix, hipStreamSynchronize(ln.s));   // only this lane's stream uses them
        if (f.dp_cnt) (void)hipFree(f.dp_cnt);
        f.dp_cnt = nullptr;
        f.dp_cap = 0;
        const uint64_t c = std::max<uint64_t>(std::min<uint64_t>(cap + cap / 4, 0xFFFFFFFFull), 4096);
        if (hipMalloc(&f.dp_cnt, c * 4) != hipSuccess) {
            (void)hipGetLastError();
            f.dp_cnt = nullptr;
            return fail(ix, TM_ENOMEM, "dispatch: no device memory for the entries' list lengths (4 bytes x cap)");
        }
        f.dp_cap = c;
    }
    if (offsets && !(cap <= f.dp_off_cap && f.dp_off)) {
        HIPCHK(ix, hipStreamSynchronize(ln.s));
        if (f.dp_off) (void)hipFree(f.dp_off);
        f.dp_off = nullptr;
        f.dp_off_cap = 0;
        const uint64_t c = std::max<uint64_t>(std::min<uint64_t>(cap + cap / 4, 0xFFFFFFFFull), 4096);
        if (hipMalloc(&f.dp_off, (c + 1) * 8) != hipSuccess) {
            (void)hipGetLastError();
            f.dp_off = nullptr;
            return fail(ix, TM_ENOMEM, "dispatch: no device memory for the delivery offsets (8 bytes x (cap + 1))");
        }
        f.dp_off_cap = c;
    }
    return TM_OK;
}

// the pick's scratch on a lane (grow-only; freed with the lane): the digit
// passes' table (the fan-out's), the block counts, and five words per entry
// below cap -- the ranked entries' slots and the two (slot, q) pair arrays
int ensure_share(tm_index *ix, Lane &ln, uint64_t cap) {
    FanoutScratch &f = ln.f;
    if (!f.tab) {
        HIPCHK(ix, hipMalloc(&f.tab, (uint64_t)FO_BINS * FO_GRID * 4));
        HIPCHK(ix, hipMalloc(&f.tot, FO_BINS * 4));
    }
    if (!f.sh_cnt && hipMalloc(&f.sh_cnt, (3ull * FO_GRID + 1) * 4) != hipSuccess) {
        (void)hipGetLastError();
        f.sh_cnt = nullptr;
        return fail(ix, TM_ENOMEM, "share pick: no device memory for the pass's block counts (48 KiB)");
    }
    if (cap <= f.sh_cap && f.sh_key) return TM_OK;
    HIPCHK(ix, hipStreamSynchronize(ln.s));   // only this lane's stream uses them
    if (f.sh_key) (void)hipFree(f.sh_key);
    f.sh_key = nullptr;
    f.sh_cap = 0;
    const uint64_t c = std::max<uint64_t>(std::min<uint64_t>(cap + cap / 4, 0xFFFFFFFFull), 4096);
    if (hipMalloc(&f.sh_key, c * 20) != hipSuccess) {
        (void)hipGetLastError();
        f.sh_key = nullptr;
        return fail(ix, TM_ENOMEM, "share pick: no device memory for the batch's scratch (20 bytes x cap)");
    }
    f.sh_s[0] = f.sh_key + c;
    f.sh_q[0] = f.sh_key + 2 * c;
    f.sh_s[1] = f.sh_key + 3 * c;
    f.sh_q[1] = f.sh_key + 4 * c;
    f.sh_cap = c;
    return TM_OK;
}

// the grouping's scratch on a lane (grow-only; freed with the lane): the fixed
// words (its counters zero) and the two (key, position) pair arrays below cap;
// who: the entry point called, for the messages
int ensure_group(tm_index *ix, Lane &ln, uint64_t cap, const char *who) {
    FanoutScratch &f = ln.f;
    if (!f.gs_fix) {
        if (hipMalloc(&f.gs_fix, (uint64_t)GS_FIX_WORDS * 4) != hipSuccess) {
            (void)hipGetLastError();
            f.gs_fix = nullptr;
            return fail(ix, TM_ENOMEM, std::string(who) + ": no device memory for the grouping's histograms (1.1 MiB)");
        }
        HIPCHK(ix, hipMemsetAsync(f.gs_fix, 0, (uint64_t)GS_ZERO_WORDS * 4, ln.s));   // the pass counters, the bin totals
    }
    if (cap <= f.gs_cap && f.gs_k[0]) return TM_OK;
    HIPCHK(ix, hipStreamSynchronize(ln.s));   // only this lane's stream uses them
    if (f.gs_k[0]) (void)hipFree(f.gs_k[0]);
    f.gs_k[0] = nullptr;
    f.gs_cap = 0;
    const uint64_t c = std::max<uint64_t>(std::min<uint64_t>(cap + cap / 4, 0xFFFFFFFFull), 4096);
    if (hipMalloc(&f.gs_k[0], c * 16) != hipSuccess) {
        (void)hipGetLastError();
        f.gs_k[0] = nullptr;
        return fail(ix, TM_ENOMEM, std::string(who) + ": no device memory for the grouping's pair arrays (16 bytes x cap)");
    }
    f.gs_p[0] = f.gs_k[0] + c;
    f.gs_k[1] = f.gs_k[0] + 2 * c;
    f.gs_p[1] = f.gs_k[0] + 3 * c;
    f.gs_cap = c;
    return TM_OK;
}

// the scratch of the picks' merge on a lane (grow-only; freed with the lane):
// one allocation -- the fixed words, four merged arrays below `all` (cap +
// ecap), three compacted pick arrays below ecap
int ensure_group_picks(tm_index *ix, Lane &ln, uint64_t all, uint64_t ecap, const char *who) {
    FanoutScratch &f = ln.f;
    if (f.gp_fix && all <= f.gp_cap && ecap <= f.gp_ecap) return TM_OK;
    HIPCHK(ix, hipStreamSynchronize(ln.s));   // only this lane's stream uses them
    if (f.gp_fix) (void)hipFree(f.gp_fix);
    f.gp_fix = nullptr;
    const uint64_t c = std::max<uint64_t>({std::min<uint64_t>(all + all / 4, 0xFFFFFFFFull), f.gp_cap, 4096});
    const uint64_t e = std::max<uint64_t>({std::min<uint64_t>(ecap + ecap / 4, 0xFFFFFFFFull), f.gp_ecap, 4096});
    f.gp_cap = f.gp_ecap = 0;
    const uint64_t fixw = ((uint64_t)GP_FIX_WORDS + 63) & ~63ull;
    if (hipMalloc(&f.gp_fix, (fixw + 4 * c + 3 * e) * 4) != hipSuccess) {
        (void)hipGetLastError();
        f.gp_fix = nullptr;
        return fail(ix, TM_ENOMEM, std::string(who) + ": no device memory for the merge's arrays (16 bytes x (cap + ecap) "
                                                      "and 12 bytes x ecap)");
    }
    for (int i = 0; i < 4; i++) f.gp_m[i] = f.gp_fix + fixw + (uint64_t)i * c;
    for (int i = 0; i < 3; i++) f.gp_c[i] = f.gp_fix + fixw + 4 * c + (uint64_t)i * e;
    f.gp_cap = c;
    f.gp_ecap = e;
    return TM_OK;
}

// the index's member -> local subscriber table (tm_set_member_subs) on group g
int msub_upload(tm_index *ix, int g, hipStream_t s, const uint32_t *&d, uint64_t &len) {
    return table_upload(ix, ix->msub_h, ix->msub[g], g, s, d, len);
}

// the passes the live lanes' grouping calls ran (which 0) / skipped (1) so far
// (caller holds ix->mu; waits for nothing: a call still in flight is not counted)
int group_passes(tm_index *ix, int which, uint64_t &out) {
    out = 0;
    int dev = 0;
    HIPCHK(ix, hipGetDevice(&dev));
    for (auto &l : ix->lanes) {
        if (!l->f.gs_fix) continue;
        uint64_t st[2] = {0, 0};
        HIPCHK(ix, hipSetDevice(ix->rep[l->r].device));
        HIPCHK(ix, hipMemcpy(st, l->f.gs_fix + GS_STAT, 16, hipMemcpyDeviceToHost));
        out += st[which];
    }
    HIPCHK(ix, hipSetDevice(dev));
    return TM_OK;
}

// group g's state array holds `need` slots (caller holds ix->mu and
// ix->dst_mu; the calling thread is on the group's device).  It grows with
// its contents kept and the new words UNDEF: no pick may still use the old
// array, so the group's lanes with a batch in flight are waited for first.
int share_state_grow(tm_index *ix, int g, uint64_t need) {
    auto &S = ix->share_state[g];
    if (need <= S.cap) return TM_OK;
    for (auto &l : ix->lanes)
        if (ix->rep[l->r].group == g && lane_busy(*l)) HIPCHK(ix, hipEventSynchronize(l->done));
    const uint64_t c = std::max<uint64_t>(need + need / 2, 4096);
    uint32_t *nd = nullptr;
    if (hipMalloc(&nd, c * 4) != hipSuccess) {
        (void)hipGetLastError();
        return fail(ix, TM_ENOMEM, "share state: no device memory for the slots' state words (4 bytes x slots)");
    }
    hipError_t e = hipMemset(nd, 0xFF, c * 4);
    if (e == hipSuccess && S.d) e = hipMemcpy(nd, S.d, S.cap * 4, hipMemcpyDeviceToDevice);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);   // (before any lane's stream reads it)
    if (e != hipSuccess) {
        (void)hipFree(nd);
        HIPCHK(ix, e);
    }
    if (S.d) HIPCHK(ix, hipFree(S.d));
    S.d = nd;
    S.cap = c;
    return TM_OK;
}

// the index's shared-subscription tables on group g, for a pick about to be
// queued on stream s: the pool, the slot records, the value -> slot table, in
// one hold of the lock (subs_upload's reason), and the state array grown to
// the records' slots.  slot_len in values, n_slots in records.
int share_upload(tm_index *ix, int g, hipStream_t s, const uint32_t *&slot_of, uint64_t &slot_len, const uint32_t *&rec,
                 uint64_t &n_slots, const uint32_t *&pool, uint64_t &pool_len, uint32_t *&state) {
    std::lock_guard<std::mutex> dg(ix->dst_mu);
    if (int rc = table_upload_locked(ix, ix->share_h.pool, ix->share_pool[g], g, s, pool, pool_len)) return rc;
    if (int rc = table_upload_locked(ix, ix->share_rec_h, ix->share_rec[g], g, s, rec, n_slots)) return rc;
    if (int rc = table_upload_locked(ix, ix->share_slot_h, ix->share_slot[g], g, s, slot_of, slot_len)) return rc;
    n_slots /= 4;
    if (int rc = share_state_grow(ix, g, n_slots)) return rc;
    state = ix->share_state[g].d;
    return TM_OK;
}

// the calling thread's HIP device, put back when the scope ends
struct DeviceScope {
    int dev = -1;
    DeviceScope() { if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); dev = -1; } }
    ~DeviceScope() { if (dev >= 0) (void)hipSetDevice(dev); }
};

int group_device(tm_index *ix, int g) {
    for (int r = 0; r < ix->nrep; r++)
        if (ix->rep[r].group == g) return ix->rep[r].device;
    return ix->rep[0].device;
}

// every batch queued on group g so far is over (caller holds ix->mu)
int drain_group(tm_index *ix, int g) {
    for (auto &l : ix->lanes)
        if (ix->rep[l->r].group == g && lane_busy(*l)) HIPCHK(ix, hipEventSynchronize(l->done));
    return TM_OK;
}

// tm_set_dests / tm_set_route_filters: n entries into a host table and every
// group's dirty range
int table_set(tm_index *ix, std::vector<uint32_t> &host, tm_index::DestDev *dev, uint64_t n, const uint32_t *values,
              const uint32_t *what, const char *oom) {
    std::lock_guard<std::mutex> dg(ix->dst_mu);
    uint64_t lo = UINT64_MAX, hi = 0;
    for (uint64_t i = 0; i < n; i++) {
        lo = std::min<uint64_t>(lo, values[i]);
        hi = std::max<uint64_t>(hi, (uint64_t)values[i] + 1);
    }
    if (hi > host.size()) {
        // the entries between the old end and the lowest new value become NONE
        // on the host: they go up too, so no device entry below `len` is ever
        // one the host never wrote
        lo = std::min<uint64_t>(lo, host.size());
        try {
            host.resize(hi, NONE);
        } catch (const std::bad_alloc &) {
            return fail(ix, TM_ENOMEM, oom);
        }
    }
    for (uint64_t i = 0; i < n; i++) host[values[i]] = what[i];
    for (int g = 0; g < ix->ngroups; g++) {
        auto &D = dev[g];
        if (D.hi > D.lo) {
            D.lo = std::min(D.lo, lo);
            D.hi = std::max(D.hi, hi);
        } else {
            D.lo = lo;
            D.hi = hi;
        }
    }
    return TM_OK;
}

// the aggre pass's scratch on a lane (grow-only; freed with the lane): a
// bitmap word and a base per 64 positions below cap, the block counts
int ensure_aggre(tm_index *ix, Lane &ln, uint64_t cap) {
    FanoutScratch &f = ln.f;
    if (!f.ag_cnt && hipMalloc(&f.ag_cnt, ((uint64_t)FO_GRID + 1) * 4) != hipSuccess) {
        (void)hipGetLastError();
        f.ag_cnt = nullptr;
        return fail(ix, TM_ENOMEM, "aggre: no device memory for the pass's block counts (16 KiB)");
    }
    if (cap <= f.ag_cap && f.ag_bits) return TM_OK;
    HIPCHK(ix, hipStreamSynchronize(ln.s));   // only this lane's stream uses them
    if (f.ag_bits) (void)hipFree(f.ag_bits);
    if (f.ag_pre) (void)hipFree(f.ag_pre);
    f.ag_bits = nullptr;
    f.ag_pre = nullptr;
    f.ag_cap = 0;
    const uint64_t c = std::max<uint64_t>(std::min<uint64_t>(cap + cap / 4, 0xFFFFFFFFull), 4096);
    const uint64_t words = (c + 63) / 64;
    if (hipMalloc(&f.ag_bits, words * 8) != hipSuccess || hipMalloc(&f.ag_pre, words * 4) != hipSuccess) {
        (void)hipGetLastError();
        if (f.ag_bits) (void)hipFree(f.ag_bits);
        f.ag_bits = nullptr;
        return fail(ix, TM_ENOMEM, "aggre: no device memory for the pass's scratch (12 bytes x cap / 64)");
    }
    f.ag_cap = c;
    return TM_OK;
}

}  // namespace

extern "C" {

int tm_set_dests(tm_index *ix, uint64_t n, const uint32_t *values, const uint32_t *dests) {
    if (!ix) return fail(nullptr, TM_EINVAL, "tm_set_dests: null handle");
    if (n && (!values || !dests)) return fail(ix, TM_EINVAL, "tm_set_dests: null buffer");
    if (!n) return TM_OK;
    return table_set(ix, ix->dest_h, ix->dest, n, values, dests,
                     "tm_set_dests: out of host memory (the table has one entry per value up to the largest)");
}

int tm_set_member_subs(tm_index *ix, uint64_t n, const uint32_t *members, const uint32_t *sub_ids) {
    if (!ix) return fail(nullptr, TM_EINVAL, "tm_set_member_subs: null handle");
    if (n && (!members || !sub_ids)) return fail(ix, TM_EINVAL, "tm_set_member_subs: null buffer");
    if (!n) return TM_OK;
    return table_set(ix, ix->msub_h, ix->msub, n, members, sub_ids,
                     "tm_set_member_subs: out of host memory (the table has one entry per member id up to the largest)");
}

int tm_set_route_filters(tm_index *ix, uint64_t n, const uint32_t *values, const uint32_t *filter_ids) {
    if (!ix) return fail(nullptr, TM_EINVAL, "tm_set_route_filters: null handle");
    if (n && (!values || !filter_ids)) return fail(ix, TM_EINVAL, "tm_set_route_filters: null buffer");
    if (!n) return TM_OK;
    return table_set(ix, ix->filt_h, ix->filt, n, values, filter_ids,
                     "tm_set_route_filters: out of host memory (the table has one entry per value up to the largest)");
}

int tm_set_subscribers(tm_index *ix, uint64_t n, const uint32_t *values, const uint64_t *list_offsets,
                       const uint32_t *subs) {
    if (!ix) return fail(nullptr, TM_EINVAL, "tm_set_subscribers: null handle");
    if (n && (!values || !list_offsets)) return fail(ix, TM_EINVAL, "tm_set_subscribers: null buffer");
    if (!n) return TM_OK;
    for (uint64_t i = 0; i < n; i++) {
        if (list_offsets[i + 1] < list_offsets[i]) return fail(ix, TM_EINVAL, "tm_set_subscribers: decreasing offsets");
        if (list_offsets[i + 1] - list_offsets[i] > 0xFFFFFFFFull)
            return fail(ix, TM_EINVAL, "tm_set_subscribers: a list of more than 2^32 - 1 subscribers");
    }
    if (list_offsets[n] > list_offsets[0] && !subs) return fail(ix, TM_EINVAL, "tm_set_subscribers: null buffer");
    std::lock_guard<std::mutex> dg(ix->dst_mu);
    SubPool &sp = ix->subs_h;
    bool ok = true;
    try {
        for (uint64_t i = 0; i < n && ok; i++)
            ok = sp.set(values[i], subs + list_offsets[i], (uint32_t)(list_offsets[i + 1] - list_offsets[i]));
    } catch (const std::bad_alloc &) {
        ok = false;
    }
    // (what was written before a failure is written: the device copies follow it)
    uint64_t slo, shi, plo, phi;
    bool whole;
    sp.take_dirty(slo, shi, plo, phi, whole);
    for (int g = 0; g < ix->ngroups; g++) {
        auto &S = ix->sub_span[g], &P = ix->sub_pool[g];
        if (whole) {   // compacted: the pool may have shrunk under an older range
            S.lo = P.lo = 0;
            S.hi = sp.span.size();
            P.hi = sp.pool.size();
        } else {
            SubPool::widen(S.lo, S.hi, slo, shi);
            SubPool::widen(P.lo, P.hi, plo, phi);
        }
    }
    if (!ok)
        return fail(ix, TM_ENOMEM, "tm_set_subscribers: out of host memory (a span per value up to the largest, the "
                                   "lists in a pool of at most 2^32 - 1 words)");
    return TM_OK;
}

int tm_dispatch_dev(tm_index *ix, uint32_t n_dests, const uint64_t *dest_offs, uint32_t bucket, const uint32_t *topic,
                    const uint32_t *value, uint64_t cap, const uint32_t *sub_span, uint64_t span_len,
                    const uint32_t *sub_pool, uint64_t pool_len, uint64_t *out_head, uint64_t *out_offsets,
                    uint32_t *out_topic, uint32_t *out_value, uint32_t *out_sub, uint64_t out_cap, void *stream) {
    if (!ix) return fail(nullptr, TM_EINVAL, "tm_dispatch_dev: null handle");
    if (!n_dests || n_dests > FO_MAX_DESTS) return fail(ix, TM_EINVAL, "tm_dispatch_dev: n_dests must be 1 .. 65536");
    if (bucket > n_dests) return fail(ix, TM_EINVAL, "tm_dispatch_dev: bucket must be 0 .. n_dests");
    if (!dest_offs || !out_head || (cap && (!topic || !value)) || (out_cap && (!out_topic || !out_value || !out_sub)))
        return fail(ix, TM_EINVAL, "tm_dispatch_dev: null buffer");
    if (sub_span && !sub_pool && pool_len) return fail(ix, TM_EINVAL, "tm_dispatch_dev: d_sub_span without d_sub_pool");
    if ((uintptr_t)sub_span & 7) return fail(ix, TM_EINVAL, "tm_dispatch_dev: d_sub_span must be 8-byte aligned");
    if (cap > 0xFFFFFFFFull) cap = 0xFFFFFFFFull;   // (32-bit positions)
    if (out_cap > 0xFFFFFFFFull) out_cap = 0xFFFFFFFFull;
    DevBatch b(ix, stream);
    int rc;
    if ((rc = b.open_fanout())) return rc;
    if ((rc = ensure_dispatch(ix, *b.ln, cap, !out_offsets))) return rc;
    if (!sub_span && (rc = subs_upload(ix, b.grp, b.s, sub_span, span_len, sub_pool, pool_len))) return rc;
    HIPCHK(ix, launch_dispatch(b.ln->f, n_dests, dest_offs, bucket, topic, value, cap, sub_span, span_len, sub_pool,
                               pool_len, out_head, out_offsets, out_topic, out_value, out_sub, out_cap, b.s));
    return b.done();
}

int tm_group_subs_dev(tm_index *ix, const uint64_t *head, const uint32_t *topic, const uint32_t *value,
                      const uint32_t *sub, uint64_t cap, uint64_t *out_ghead, uint32_t *out_gsub, uint64_t *out_goff,
                      uint64_t gcap, uint32_t *out_topic, uint32_t *out_value, uint32_t *out_sub, uint32_t *out_perm,
                      void *stream) {
    if (!ix) return fail(nullptr, TM_EINVAL, "tm_group_subs_dev: null handle");
    if (!head || !out_ghead || !out_goff || (gcap && !out_gsub) ||
        (cap && (!topic || !value || !sub || !out_topic || !out_value || !out_sub)))
        return fail(ix, TM_EINVAL, "tm_group_subs_dev: null buffer");
    if ((uintptr_t)head & 7) return fail(ix, TM_EINVAL, "tm_group_subs_dev: d_head must be 8-byte aligned");
    if ((uintptr_t)out_ghead & 7) return fail(ix, TM_EINVAL, "tm_group_subs_dev: d_out_ghead must be 8-byte aligned");
    if ((uintptr_t)out_goff & 7) return fail(ix, TM_EINVAL, "tm_group_subs_dev: d_out_goff must be 8-byte aligned");
    if (cap > 0xFFFFFFFFull) cap = 0xFFFFFFFFull;   // (32-bit positions)
    DevBatch b(ix, stream);
    int rc;
    if ((rc = b.open_fanout())) return rc;
    if ((rc = ensure_group(ix, *b.ln, cap, "tm_group_subs_dev"))) return rc;
    HIPCHK(ix, launch_group_subs(b.ln->f, head, topic, value, sub, cap, out_ghead, out_gsub, out_goff, gcap, out_topic,
                                 out_value, out_sub, out_perm, b.s));
    return b.done();
}

int tm_group_picks_dev(tm_index *ix, const uint64_t *head, const uint32_t *topic, const uint32_t *value,
                       const uint32_t *sub, uint64_t cap, uint32_t n_dests, const uint64_t *dest_offs,
                       const uint32_t *etopic, const uint32_t *evalue, const uint32_t *member, uint64_t ecap,
                       const uint32_t *sub_of, uint64_t sub_of_len, uint64_t *out_ghead, uint32_t *out_gsub,
                       uint64_t *out_goff, uint64_t gcap, uint32_t *out_topic, uint32_t *out_value, uint32_t *out_sub,
                       uint32_t *out_src, uint64_t out_cap, void *stream) {
    if (!ix) return fail(nullptr, TM_EINVAL, "tm_group_picks_dev: null handle");
    if (!n_dests || n_dests > FO_MAX_DESTS) return fail(ix, TM_EINVAL, "tm_group_picks_dev: n_dests must be 1 .. 65536");
    if (cap > 0xFFFFFFFFull) cap = 0xFFFFFFFFull;   // (32-bit positions)
    if (ecap > 0xFFFFFFFFull) ecap = 0xFFFFFFFFull;
    if (out_cap > 0xFFFFFFFFull) out_cap = 0xFFFFFFFFull;
    if (!head || !dest_offs || !out_ghead || !out_goff || (gcap && !out_gsub) || (cap && (!topic || !value || !sub)) ||
        (ecap && (!etopic || !evalue || !member)) || (out_cap && (!out_topic || !out_value || !out_sub)))
        return fail(ix, TM_EINVAL, "tm_group_picks_dev: null buffer");
    if ((uintptr_t)head & 7) return fail(ix, TM_EINVAL, "tm_group_picks_dev: d_head must be 8-byte aligned");
    if ((uintptr_t)dest_offs & 7) return fail(ix, TM_EINVAL, "tm_group_picks_dev: d_dest_offsets must be 8-byte aligned");
    if ((uintptr_t)out_ghead & 7) return fail(ix, TM_EINVAL, "tm_group_picks_dev: d_out_ghead must be 8-byte aligned");
    if ((uintptr_t)out_goff & 7) return fail(ix, TM_EINVAL, "tm_group_picks_dev: d_out_goff must be 8-byte aligned");
    if (sub_of && sub_of_len > 0xFFFFFFFFull) return fail(ix, TM_EINVAL, "tm_group_picks_dev: more than 2^32 - 1 members");
    if (cap + ecap > 0xFFFFFFFFull)
        return fail(ix, TM_EINVAL, "tm_group_picks_dev: cap + ecap must be at most 2^32 - 1 (32-bit positions)");
    DevBatch b(ix, stream);
    int rc;
    if ((rc = b.open_fanout())) return rc;
    if ((rc = ensure_group(ix, *b.ln, cap + ecap, "tm_group_picks_dev"))) return rc;
    if ((rc = ensure_group_picks(ix, *b.ln, cap + ecap, ecap, "tm_group_picks_dev"))) return rc;
    if (!sub_of && (rc = msub_upload(ix, b.grp, b.s, sub_of, sub_of_len))) return rc;
    HIPCHK(ix, launch_group_picks(b.ln->f, head, topic, value, sub, cap, n_dests, dest_offs, etopic, evalue, member, ecap,
                                  sub_of, sub_of_len, out_ghead, out_gsub, out_goff, gcap, out_topic, out_value, out_sub,
                                  out_src, out_cap, GS_PASSES, b.s));
    return b.done();
}

int tm_set_share_slots(tm_index *ix, uint64_t n, const uint32_t *values, const uint32_t *slots) {
    if (!ix) return fail(nullptr, TM_EINVAL, "tm_set_share_slots: null handle");
    if (n && (!values || !slots)) return fail(ix, TM_EINVAL, "tm_set_share_slots: null buffer");
    if (!n) return TM_OK;
    return table_set(ix, ix->share_slot_h, ix->share_slot, n, values, slots,
                     "tm_set_share_slots: out of host memory (the table has one entry per value up to the largest)");
}

int tm_set_share_members(tm_index *ix, uint64_t n, const uint32_t *slots, const uint64_t *list_offsets,
                         const uint32_t *members, const uint32_t *n_local, const uint32_t *meta) {
    if (!ix) return fail(nullptr, TM_EINVAL, "tm_set_share_members: null handle");
    if (n && (!slots || !list_offsets || !n_local || !meta))
        return fail(ix, TM_EINVAL, "tm_set_share_members: null buffer");
    if (!n) return TM_OK;
    for (uint64_t i = 0; i < n; i++) {
        if (slots[i] == NONE) return fail(ix, TM_EINVAL, "tm_set_share_members: slot 0xFFFFFFFF means none");
        if (list_offsets[i + 1] < list_offsets[i]) return fail(ix, TM_EINVAL, "tm_set_share_members: decreasing offsets");
        if (list_offsets[i + 1] - list_offsets[i] > 0xFFFFFFFFull)
            return fail(ix, TM_EINVAL, "tm_set_share_members: a list of more than 2^32 - 1 members");
    }
    if (list_offsets[n] > list_offsets[0] && !members) return fail(ix, TM_EINVAL, "tm_set_share_members: null buffer");
    for (uint64_t k = list_offsets[0]; k < list_offsets[n]; k++)
        if (members[k] == NONE)
            return fail(ix, TM_EINVAL, "tm_set_share_members: member id 0xFFFFFFFF means no pick");
    std::lock_guard<std::mutex> dg(ix->dst_mu);
    SubPool &sp = ix->share_h;
    auto &rec = ix->share_rec_h;
    bool ok = true;
    uint64_t done = 0, rlo = 0, rhi = 0;
    try {
        for (; done < n && ok; done += ok)
            ok = sp.set(slots[done], members + list_offsets[done],
                        (uint32_t)(list_offsets[done + 1] - list_offsets[done]));
        const uint64_t old = rec.size();
        rec.resize(4 * sp.values(), 0);
        SubPool::widen(rlo, rhi, old, rec.size());
    } catch (const std::bad_alloc &) {
        ok = false;
    }
    // (what was written before a failure is written: the device copies follow it)
    for (uint64_t i = 0; i < done; i++) {
        const uint64_t at = 4 * (uint64_t)slots[i];
        if (at + 4 > rec.size()) continue;   // (the records could not grow)
        rec[at + 2] = n_local[i];
        rec[at + 3] = meta[i];
        SubPool::widen(rlo, rhi, at, at + 4);
    }
    uint64_t slo, shi, plo, phi;
    bool whole;
    sp.take_dirty(slo, shi, plo, phi, whole);
    if (whole) { slo = 0; shi = sp.span.size(); }
    for (uint64_t v = slo / 2; v < (shi + 1) / 2 && 4 * v + 4 <= rec.size(); v++) {
        rec[4 * v] = sp.span[2 * v];
        rec[4 * v + 1] = sp.span[2 * v + 1];
    }
    SubPool::widen(rlo, rhi, 4 * (slo / 2), std::min<uint64_t>(4 * ((shi + 1) / 2), rec.size()));
    for (int g = 0; g < ix->ngroups; g++) {
        auto &R = ix->share_rec[g], &P = ix->share_pool[g];
        SubPool::widen(R.lo, R.hi, rlo, rhi);
        if (whole) {   // compacted: the pool may have shrunk under an older range
            P.lo = 0;
            P.hi = sp.pool.size();
        } else {
            SubPool::widen(P.lo, P.hi, plo, phi);
        }
    }
    if (!ok)
        return fail(ix, TM_ENOMEM, "tm_set_share_members: out of host memory (a record per slot up to the largest, the "
                                   "lists in a pool of at most 2^32 - 1 words)");
    return TM_OK;
}

// (slot, word) pairs in slot order, a slot named twice keeping its last word
static bool share_sorted(uint64_t n, const uint32_t *slots, const uint32_t *words,
                         std::vector<std::pair<uint32_t, uint32_t>> &out) {
    try {
        out.resize(n);
    } catch (const std::bad_alloc &) {
        return false;
    }
    for (uint64_t i = 0; i < n; i++) out[i] = {slots[i], words ? words[i] : 0u};
    std::stable_sort(out.begin(), out.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
    uint64_t k = 0;
    for (uint64_t i = 0; i < n; i++)
        if (i + 1 == n || out[i + 1].first != out[i].first) out[k++] = out[i];
    out.resize(k);
    return true;
}

int tm_share_state_set(tm_index *ix, uint64_t n, const uint32_t *slots, const uint32_t *states) {
    if (!ix) return fail(nullptr, TM_EINVAL, "tm_share_state_set: null handle");
    if (n && (!slots || !states)) return fail(ix, TM_EINVAL, "tm_share_state_set: null buffer");
    if (!n) return TM_OK;
    for (uint64_t i = 0; i < n; i++)
        if (slots[i] == NONE) return fail(ix, TM_EINVAL, "tm_share_state_set: slot 0xFFFFFFFF means none");
    std::vector<std::pair<uint32_t, uint32_t>> sw;
    std::vector<uint32_t> run;
    if (!share_sorted(n, slots, states, sw)) return fail(ix, TM_ENOMEM, "tm_share_state_set: out of host memory");
    std::lock_guard<std::mutex> g(ix->mu);
    std::lock_guard<std::mutex> dg(ix->dst_mu);
    DeviceScope scope;
    for (int grp = 0; grp < ix->ngroups; grp++) {
        HIPCHK(ix, hipSetDevice(group_device(ix, grp)));
        // after every pick queued so far, before every pick queued later: both sides wait
        if (int rc = drain_group(ix, grp)) return rc;
        if (int rc = share_state_grow(ix, grp, (uint64_t)sw.back().first + 1)) return rc;
        uint32_t *d = ix->share_state[grp].d;
        // one copy per run of consecutive slots: what is moved is bounded by n, however far apart the slots lie
        for (size_t i = 0; i < sw.size();) {
            size_t j = i + 1;
            while (j < sw.size() && sw[j].first == sw[j - 1].first + 1) j++;
            run.clear();
            for (size_t k = i; k < j; k++) run.push_back(sw[k].second);
            HIPCHK(ix, hipMemcpy(d + sw[i].first, run.data(), (j - i) * 4, hipMemcpyHostToDevice));
            i = j;
        }
        HIPCHK(ix, hipStreamSynchronize(nullptr));
    }
    return TM_OK;
}

int tm_share_state_get(tm_index *ix, uint32_t dev, uint64_t n, const uint32_t *slots, uint32_t *out) {
    if (!ix) return fail(nullptr, TM_EINVAL, "tm_share_state_get: null handle");
    if (n && (!slots || !out)) return fail(ix, TM_EINVAL, "tm_share_state_get: null buffer");
    if ((int64_t)dev >= ix->ngroups) return fail(ix, TM_EINVAL, "tm_share_state_get: no such device entry");
    if (!n) return TM_OK;
    std::vector<std::pair<uint32_t, uint32_t>> sw;   // (slot, its word once read)
    std::vector<uint32_t> run;
    if (!share_sorted(n, slots, nullptr, sw)) return fail(ix, TM_ENOMEM, "tm_share_state_get: out of host memory");
    std::lock_guard<std::mutex> g(ix->mu);
    std::lock_guard<std::mutex> dg(ix->dst_mu);
    DeviceScope scope;
    const auto &S = ix->share_state[dev];
    HIPCHK(ix, hipSetDevice(group_device(ix, (int)dev)));
    if (int rc = drain_group(ix, (int)dev)) return rc;
    for (size_t i = 0; i < sw.size();) {   // one copy per run of consecutive slots inside the array
        if (sw[i].first >= S.cap) {
            sw[i++].second = NONE;
            continue;
        }
        size_t j = i + 1;
        while (j < sw.size() && sw[j].first == sw[j - 1].first + 1 && sw[j].first < S.cap) j++;
        run.resize(j - i);
        HIPCHK(ix, hipMemcpy(run.data(), S.d + sw[i].first, (j - i) * 4, hipMemcpyDeviceToHost));
        for (size_t k = i; k < j; k++) sw[k].second = run[k - i];
        i = j;
    }
    for (uint64_t i = 0; i < n; i++) {
        const auto it = std::lower_bound(sw.begin(), sw.end(), slots[i],
                                         [](const auto &a, uint32_t v) { return a.first < v; });
        out[i] = it->second;
    }
    return TM_OK;
}

int tm_share_pick_dev(tm_index *ix, uint32_t n_dests, const uint64_t *dest_offs, const uint32_t *topic,
                      const uint32_t *value, uint64_t cap, const uint32_t *key_clientid, const uint32_t *key_topic,
                      uint64_t n_topics, uint32_t seed, const uint32_t *slot_of, uint64_t slot_of_len,
                      const uint32_t *slot_rec, uint64_t n_slots, const uint32_t *pool, uint64_t pool_len, uint32_t *state,
                      uint64_t *out_head, uint32_t *out_member, void *stream) {
    if (!ix) return fail(nullptr, TM_EINVAL, "tm_share_pick_dev: null handle");
    if (!n_dests || n_dests > FO_MAX_DESTS) return fail(ix, TM_EINVAL, "tm_share_pick_dev: n_dests must be 1 .. 65536");
    if (!dest_offs || !out_head || (cap && (!topic || !value || !out_member)))
        return fail(ix, TM_EINVAL, "tm_share_pick_dev: null buffer");
    if (slot_of) {
        if (n_slots && (!slot_rec || !state))
            return fail(ix, TM_EINVAL, "tm_share_pick_dev: d_slot_of without d_slot_rec and d_state");
        if (!pool && pool_len) return fail(ix, TM_EINVAL, "tm_share_pick_dev: d_slot_rec without d_pool");
        if ((uintptr_t)slot_rec & 15) return fail(ix, TM_EINVAL, "tm_share_pick_dev: d_slot_rec must be 16-byte aligned");
        if (n_slots > 0xFFFFFFFFull) return fail(ix, TM_EINVAL, "tm_share_pick_dev: more than 2^32 - 1 slots");
    }
    if (cap > 0xFFFFFFFFull) cap = 0xFFFFFFFFull;   // (32-bit positions)
    DevBatch b(ix, stream);
    int rc;
    if ((rc = b.open_fanout())) return rc;
    if ((rc = ensure_share(ix, *b.ln, cap))) return rc;
    if (!slot_of && (rc = share_upload(ix, b.grp, b.s, slot_of, slot_of_len, slot_rec, n_slots, pool, pool_len, state)))
        return rc;
    HIPCHK(ix, launch_share_pick(b.ln->f, n_dests, dest_offs, topic, value, cap, key_clientid, key_topic, n_topics, seed,
                                 slot_of, slot_of_len, slot_rec, n_slots, pool, pool_len, state, out_head, out_member, b.s));
    return b.done();
}

int tm_aggre_dev(tm_index *ix, uint32_t n_dests, const uint64_t *dest_offs, const uint32_t *topic, const uint32_t *value,
                 uint64_t cap, const uint32_t *filter_of, uint64_t filter_len, uint64_t *out_dest_offs,
                 uint32_t *out_topic, uint32_t *out_value, void *stream) {
    if (!ix) return fail(nullptr, TM_EINVAL, "tm_aggre_dev: null handle");
    if (!n_dests || n_dests > FO_MAX_DESTS) return fail(ix, TM_EINVAL, "tm_aggre_dev: n_dests must be 1 .. 65536");
    if (!dest_offs || !out_dest_offs || (cap && (!topic || !value || !out_topic || !out_value)))
        return fail(ix, TM_EINVAL, "tm_aggre_dev: null buffer");
    if (cap > 0xFFFFFFFFull) cap = 0xFFFFFFFFull;   // (32-bit positions)
    DevBatch b(ix, stream);
    int rc;
    if ((rc = b.open_fanout())) return rc;
    if ((rc = ensure_aggre(ix, *b.ln, cap))) return rc;
    if (!filter_of && (rc = filter_upload(ix, b.grp, b.s, filter_of, filter_len))) return rc;
    HIPCHK(ix, launch_aggre(b.ln->f, n_dests, dest_offs, topic, value, cap, filter_of, filter_len, out_dest_offs,
                            out_topic, out_value, b.s));
    return b.done();
}

int tm_fanout_dev(tm_index *ix, uint64_t n, const uint64_t *hit_offs, const uint32_t *vals, uint64_t cap,
                  const uint32_t *dest_of, uint64_t dest_len, uint32_t n_dests, uint64_t *dest_offs,
                  uint32_t *out_topic, uint32_t *out_value, void *stream) {
    if (!ix) return fail(nullptr, TM_EINVAL, "tm_fanout_dev: null handle");
    if (!n_dests || n_dests > FO_MAX_DESTS) return fail(ix, TM_EINVAL, "tm_fanout_dev: n_dests must be 1 .. 65536");
    if (!hit_offs || !dest_offs || (cap && (!vals || !out_topic || !out_value)))
        return fail(ix, TM_EINVAL, "tm_fanout_dev: null buffer");
    if (n >= 0xFFFFFFFFull) return fail(ix, TM_EINVAL, "tm_fanout_dev: too many topics");
    if (cap > 0xFFFFFFFFull) cap = 0xFFFFFFFFull;   // (32-bit positions)
    DevBatch b(ix, stream);
    int rc;
    if ((rc = b.open_fanout())) return rc;
    if ((rc = ensure_fanout(ix, *b.ln, n_dests, cap))) return rc;
    if (!dest_of && (rc = dest_upload(ix, b.grp, b.s, dest_of, dest_len))) return rc;
    HIPCHK(ix, launch_fanout(b.ln->f, n, hit_offs, vals, cap, dest_of, dest_len, n_dests, dest_offs, out_topic, out_value,
                             b.s));
    return b.done();
}

int tm_fanout_dev_pairs(tm_index *ix, uint64_t n, const uint32_t *pairs, const uint32_t *vals, uint64_t cap,
                        const uint32_t *dest_of, uint64_t dest_len, uint32_t n_dests, uint64_t *dest_offs,
                        uint32_t *out_topic, uint32_t *out_value, void *stream) {
    if (!ix) return fail(nullptr, TM_EINVAL, "tm_fanout_dev_pairs: null handle");
    if (!n_dests || n_dests > FO_MAX_DESTS) return fail(ix, TM_EINVAL, "tm_fanout_dev_pairs: n_dests must be 1 .. 65536");
    if (!pairs || !dest_offs || (cap && (!vals || !out_topic || !out_value)))
        return fail(ix, TM_EINVAL, "tm_fanout_dev_pairs: null buffer");
    if ((uintptr_t)pairs & 7) return fail(ix, TM_EINVAL, "tm_fanout_dev_pairs: d_pairs must be 8-byte aligned");
    if (n >= 0xFFFFFFFFull) return fail(ix, TM_EINVAL, "tm_fanout_dev_pairs: too many topics");
    if (cap > 0xFFFFFFFFull) cap = 0xFFFFFFFFull;   // (32-bit positions)
    DevBatch b(ix, stream);
    int rc;
    if ((rc = b.open_fanout())) return rc;
    if ((rc = ensure_fanout(ix, *b.ln, n_dests, cap, true, n))) return rc;
    if (!dest_of && (rc = dest_upload(ix, b.grp, b.s, dest_of, dest_len))) return rc;
    HIPCHK(ix, launch_fanout_pairs(b.ln->f, n, pairs, vals, cap, dest_of, dest_len, n_dests, dest_offs, out_topic,
                                   out_value, b.s));
    return b.done();
}

int tm_stream_release(tm_index *ix, void *stream) {
    if (!ix) return fail(nullptr, TM_EINVAL, "tm_stream_release: null handle");
    std::lock_guard<std::mutex> g(ix->mu);
    hipStream_t s = pick_stream(ix, stream);
    int dev = 0;
    HIPCHK(ix, hipGetDevice(&dev));
    for (size_t i = 0; i < ix->lanes.size(); i++) {
        Lane &l = *ix->lanes[i];
        if (l.owned || l.s != s || ix->rep[l.r].device != dev) continue;
        if (l.used) HIPCHK(ix, hipEventSynchronize(l.done));
        free_lane(l);
        ix->lanes.erase(ix->lanes.begin() + i);
        break;
    }
    return TM_OK;
}

namespace {

// Batches of up to ZC_TOPICS topics are staged zero-copy: the kernels read the
// topics from, and write offsets / flags / values into, mapped pinned host
// memory over PCIe.  A small batch then costs its kernels plus one host
// synchronisation -- no copy commands and no gaps between them.  Larger
// batches move in one H2D and one D2H transfer.
constexpr uint64_t ZC_TOPICS = 65536;

int pin_mapped(tm_index *ix, hipStream_t s, uint8_t *&host, uint8_t *&dev, uint64_t &cap, uint64_t need) {
    if (need <= cap) return TM_OK;
    HIPCHK(ix, hipStreamSynchronize(s));
    if (host) HIPCHK(ix, hipHostFree(host));
    host = dev = nullptr;
    cap = need + need / 4;
    HIPCHK(ix, hipHostMalloc(&host, cap, hipHostMallocMapped));
    HIPCHK(ix, hipHostGetDevicePointer(reinterpret_cast<void **>(&dev), host, 0));
    return TM_OK;
}

// the TM_ALLOC_VRAM buffer holding [p, p + bytes), or null (caller holds ix->mu)
const tm_index::Pinned *vram_buf(tm_index *ix, const void *p, uint64_t bytes) {
    const uint8_t *q = static_cast<const uint8_t *>(p);
    for (const auto &b : ix->pinned)
        if (b.vram && q >= b.host && bytes <= b.size && q - b.host <= (ptrdiff_t)(b.size - bytes)) return &b;
    return nullptr;
}

// A host topic batch -> what the kernels read: rebased offsets, then the bytes
// (16-aligned: the walk's aligned 16-byte loads), in one buffer of the lane.
// Inputs in TM_ALLOC_VRAM memory are read where they lie, never by the host
// (each host read of it is an uncached PCIe round trip, ~0.6 us):
// bytes there are used in place with the offsets unrebased; u64 offsets there
// too are used in place; u32 offsets there (to32v, the 32-bit API) are widened
// by a kernel into the lane's scratch.  Only `to[0]`/`to[n]` (or to32v[n])
// are read by the host for a VRAM batch.
int stage_in(tm_index *ix, Lane &ln, uint64_t n, const uint8_t *tb, const uint64_t *to, const uint32_t *to32v,
             const uint8_t *&dbytes, const uint64_t *&doffs) {
    int rc;
    const uint64_t end = to32v ? to32v[n] : to[n];
    const uint64_t b0 = to32v ? 0 : to[0];
    const bool vbytes = vram_buf(ix, tb, std::max<uint64_t>(end, 1)) != nullptr;
    const bool voffs = to32v || vram_buf(ix, to, (n + 1) * 8) != nullptr;
    if (vbytes && voffs) {   // both in HBM already: nothing crosses PCIe
        dbytes = tb;
        if (to32v) {
            if ((rc = grow_dev(ix, ln.s, ln.d_o64, ln.d_o64_cap, n + 1))) return rc;
            HIPCHK(ix, launch_offs_widen(to32v, ln.d_o64, n + 1, ln.s));
            doffs = ln.d_o64;
        } else {
            doffs = to;
        }
        return TM_OK;
    }
    if (to32v || voffs) {   // offsets in HBM, bytes in host memory (no caller of the library does this)
        uint64_t *o = nullptr;
        if ((rc = pin_mapped(ix, ln.s, ln.pin_in, ln.pin_in_dev, ln.pin_in_cap, (n + 1) * 8 + end + 32))) return rc;
        o = reinterpret_cast<uint64_t *>(ln.pin_in);
        if (to32v) HIPCHK(ix, launch_offs_widen(to32v, reinterpret_cast<uint64_t *>(ln.pin_in_dev), n + 1, ln.s));
        else HIPCHK(ix, hipMemcpyAsync(o, to, (n + 1) * 8, hipMemcpyDeviceToHost, ln.s));
        const uint64_t boff = ((n + 1) * 8 + 15) & ~15ull;
        if (end) memcpy(ln.pin_in + boff, tb, end);   // bytes [0, end): the offsets stay unrebased
        dbytes = ln.pin_in_dev + boff;
        doffs = reinterpret_cast<const uint64_t *>(ln.pin_in_dev);
        if (n > ZC_TOPICS) {
            if ((rc = grow_dev(ix, ln.s, ln.d_in, ln.d_in_cap, boff + end + 16))) return rc;
            HIPCHK(ix, hipMemcpyAsync(ln.d_in, ln.pin_in, boff + end, hipMemcpyHostToDevice, ln.s));
            dbytes = ln.d_in + boff;
            doffs = reinterpret_cast<const uint64_t *>(ln.d_in);
        }
        return TM_OK;
    }
    const uint64_t nbytes = vbytes ? 0 : end - b0;   // bytes in HBM: only the offsets move
    const uint64_t boff = ((n + 1) * 8 + 15) & ~15ull;
    const uint64_t need = boff + nbytes + 16;
    if ((rc = pin_mapped(ix, ln.s, ln.pin_in, ln.pin_in_dev, ln.pin_in_cap, need))) return rc;
    uint64_t *po = reinterpret_cast<uint64_t *>(ln.pin_in);
    const uint64_t rb = vbytes ? 0 : b0;
    for (uint64_t i = 0; i <= n; i++) po[i] = to[i] - rb;
    if (nbytes) memcpy(ln.pin_in + boff, tb + b0, nbytes);
    const uint8_t *base = ln.pin_in_dev;
    if (n > ZC_TOPICS) {
        if ((rc = grow_dev(ix, ln.s, ln.d_in, ln.d_in_cap, need))) return rc;
        HIPCHK(ix, hipMemcpyAsync(ln.d_in, ln.pin_in, boff + nbytes, hipMemcpyHostToDevice, ln.s));
        base = ln.d_in;
    }
    doffs = reinterpret_cast<const uint64_t *>(base);
    dbytes = vbytes ? tb : base + boff;
    return TM_OK;
}

// where the kernels write `bytes` of per-topic results (read back by fetch_out)
int stage_out(tm_index *ix, Lane &ln, uint64_t n, uint64_t bytes, uint8_t *&dout) {
    int rc;
    if ((rc = pin_mapped(ix, ln.s, ln.pin_out, ln.pin_out_dev, ln.pin_out_cap, bytes + 16))) return rc;
    dout = ln.pin_out_dev;
    if (n > ZC_TOPICS) {
        if ((rc = grow_dev(ix, ln.s, ln.d_res, ln.d_res_cap, bytes + 16))) return rc;
        dout = ln.d_res;
    }
    return TM_OK;
}

int fetch_out(tm_index *ix, Lane &ln, uint64_t n, uint64_t bytes) {
    if (n > ZC_TOPICS && bytes) HIPCHK(ix, hipMemcpyAsync(ln.pin_out, ln.d_res, bytes, hipMemcpyDeviceToHost, ln.s));
    return TM_OK;
}

}  // namespace

// device address of [p, p + bytes) if the range lies in one tm_host_alloc buffer
static uint8_t *pinned_dev(tm_index *ix, const void *p, uint64_t bytes) {
    const uint8_t *q = static_cast<const uint8_t *>(p);
    for (const auto &b : ix->pinned)
        if (q >= b.host && bytes <= b.size && q - b.host <= (ptrdiff_t)(b.size - bytes)) return b.dev + (q - b.host);
    return nullptr;
}

int tm_host_alloc_ex(tm_index *ix, uint64_t bytes, uint32_t flags, void **out) {
    if (!ix || !out) return fail(ix, TM_EINVAL, "tm_host_alloc: null argument");
    *out = nullptr;
    if (flags & ~TM_ALLOC_VRAM) return fail(ix, TM_EINVAL, "tm_host_alloc_ex: unknown flags");
    std::lock_guard<std::mutex> g(ix->mu);
    HIPCHK(ix, hipSetDevice(ix->rep[0].device));
    void *h = nullptr, *d = nullptr;
    if (flags & TM_ALLOC_VRAM) {
        // a replica on another device would read it over the fabric: one device only
        for (int r = 1; r < ix->nrep; r++)
            if (ix->rep[r].device != ix->rep[0].device)
                return fail(ix, TM_EINVAL, "tm_host_alloc_ex: TM_ALLOC_VRAM needs a one-device index");
        // the host writes it through the PCIe BAR: only where the whole of the
        // device's memory is mapped there (large / resizable BAR) -- else a host
        // store could fault the caller; TM_EINVAL, and the caller
        // keeps its inputs in tm_host_alloc memory (the NIF does)
        int large_bar = 0;
        if (hipDeviceGetAttribute(&large_bar, hipDeviceAttributeIsLargeBar, ix->rep[0].device) != hipSuccess || !large_bar)
            return fail(ix, TM_EINVAL, "tm_host_alloc_ex: the device's memory is not mapped for the host (no large BAR)");
        // fine-grained: the host maps it through the BAR (same virtual address)
        if (hipExtMallocWithFlags(&d, bytes ? bytes : 1, hipDeviceMallocFinegrained) != hipSuccess || !d)
            return fail(ix, TM_ENOMEM, "tm_host_alloc_ex: fine-grained device allocation failed");
        hipPointerAttribute_t pa;
        if (hipPointerGetAttributes(&pa, d) != hipSuccess || pa.type != hipMemoryTypeDevice) {
            (void)hipFree(d);
            return fail(ix, TM_EINVAL, "tm_host_alloc_ex: the allocation is not device memory");
        }
        ix->pinned.push_back({static_cast<uint8_t *>(d), static_cast<uint8_t *>(d), bytes, true});
        *out = d;
        return TM_OK;
    }
    // portable: every replica's device reads it in place (one virtual address on ROCm)
    if (hipHostMalloc(&h, bytes ? bytes : 1, hipHostMallocMapped | hipHostMallocPortable) != hipSuccess || !h)
        return fail(ix, TM_ENOMEM, "tm_host_alloc: hipHostMalloc failed");
    HIPCHK(ix, hipHostGetDevicePointer(&d, h, 0));
    ix->pinned.push_back({static_cast<uint8_t *>(h), static_cast<uint8_t *>(d), bytes, false});
    *out = h;
    return TM_OK;
}

int tm_host_alloc(tm_index *ix, uint64_t bytes, void **out) { return tm_host_alloc_ex(ix, bytes, 0, out); }

int tm_host_free(tm_index *ix, void *p) {
    if (!ix) return fail(nullptr, TM_EINVAL, "tm_host_free: null handle");
    if (!p) return TM_OK;
    std::lock_guard<std::mutex> g(ix->mu);
    for (size_t i = 0; i < ix->pinned.size(); i++) {
        if (ix->pinned[i].host != p) continue;
        int rc = drain_lanes(ix);   // no batch may still read or write it
        if (rc) return rc;
        if (ix->pinned[i].vram) HIPCHK(ix, hipFree(p));
        else HIPCHK(ix, hipHostFree(p));
        ix->pinned.erase(ix->pinned.begin() + i);
        return TM_OK;
    }
    return fail(ix, TM_EINVAL, "tm_host_free: not a tm_host_alloc buffer of this index");
}

// an optional caller buffer of an in-place batch: its device address, or null
// when it is absent or empty; one that is present must lie in a tm_host_alloc
// buffer, else `ok` is cleared (the batch is staged)
static uint8_t *opt_dev(tm_index *ix, const void *p, uint64_t bytes, bool &ok) {
    if (!p || !bytes) return nullptr;
    uint8_t *d = pinned_dev(ix, p, bytes);
    if (!d) ok = false;
    return d;
}


// ---- the host-batch combiner (32-bit in-place batches, the NIF's calls)
//
// Concurrent callers' small batches run better as fewer, larger launches: a
// lone 4k batch keeps the GPU ~26 us for fixed costs a 64k batch pays once
// (host to host: 4k 0.040 ms, 64k 0.19 ms), and 8 callers' kernels do not
// overlap beyond ~3 at a time.  A caller queues its batch;
// while fewer than cmb_leaders launches are running it takes the lead: it
// takes the queued batches (in order, up to SMALL_SEGS of them and
// ZC_TOPICS topics), runs them as ONE k_walk_small launch with a segment
// table (each segment its own inputs, outputs and look-back region), and
// marks them done, waking each of their callers (one condition variable per
// request: no herd of every waiting caller per launch).  A lone caller leads
// its own batch at once: its latency is the single-batch path's.
// TM_DEBUG_CMB_GATHER (us, study knob, 0 = off): a new leader first waits up to
// that long while fewer batches are queued or in flight than the recent
// high-water mark (callers between two batches are about to queue theirs), so
// launches carry more batches.  (Round 6 measured, and removed, a landing
// variant: the launch writing its outputs to an HBM arena and one copy kernel
// moving them to the callers' buffers -- slower than the walk's in-place
// writes)
struct SmallReq {
    uint64_t n;
    const uint8_t *db; const uint8_t *dof; uint8_t *dh; uint8_t *de; uint8_t *dv;
    uint64_t cap;
    bool pairs = false;         // (offset, count) pairs out (tm_match_batch32_pairs); a launch carries one kind
    int rc = TM_OK;
    bool done = false;
    std::condition_variable cv;
    std::atomic<int> poke{0};   // done, or it may lead: a spinning waiter stops spinning
};
constexpr int CMB_LEGACY = 1;   // (not a TM_ code) the index no longer allows the one-launch path
constexpr uint64_t CMB_HW_NS = 2000000;   // the high-water mark's memory (2 ms)

static int run_small_group(tm_index *ix, const std::vector<SmallReq *> &grp, uint64_t *t_sync_end) {
    uint64_t total = 0;
    for (auto *r : grp) total += r->n;
    const uint64_t ta = g_cmb_timing ? ns_now() : 0;
    HostBatch hb(ix);
    const uint64_t tb = g_cmb_timing ? ns_now() : 0;
    int rc;
    if ((rc = hb.open(total + (uint64_t)SMALL_SEGS * SM_TOPICS))) return rc;
    Lane &ln = *hb.ln;
    if (!small_path_ok(dev_view(ix, ln.r), total)) return CMB_LEGACY;
    ix->rep[ln.r].batches++;
    SmallSegs sg{};
    sg.count = (uint32_t)grp.size();
    sg.pairs = grp[0]->pairs ? 1u : 0u;
    for (size_t k = 0; k < grp.size(); k++) {
        const SmallReq &r = *grp[k];
        const uint64_t vcap = r.dv ? r.cap : 0;
        sg.s[k] = SmallSeg{r.db ? r.db : r.dof, r.dof, r.dh, r.de, reinterpret_cast<uint32_t *>(r.dv), vcap,
                           (uint32_t)r.n, 0};
    }
    const uint64_t tc = g_cmb_timing ? ns_now() : 0;
    rc = hb.run([&](const DevIndex &d, uint32_t tag) -> int {
        int path = PATH_SMALL;
        HIPCHK(ix, launch_small_segs(d, ln.w, sg, true, tag, next_lb(ix), ix->small_kind, ln.s, &path));
        ix->path_batches[path]++;
        ix->cmb_launches++;
        ix->cmb_batches += grp.size();
        return TM_OK;
    });
    if (g_cmb_timing && hb.t_synced) {   // (the last attempt's launch and wait)
        g_cmbt.groups++;
        g_cmbt.lock_ns += tb - ta; g_cmbt.setup_ns += tc - tb;
        g_cmbt.launch_ns += hb.t_queued - tc; g_cmbt.sync_ns += hb.t_synced - hb.t_queued;
        *t_sync_end = hb.t_synced;
    }
    return rc;
}

// (caller holds cmb_mu) queued + in flight, against the recent high-water mark
static void cmb_note_load(tm_index *ix) {
    const int cur = (int)ix->cmb_q.size() + ix->cmb_inflight;
    const uint64_t t = ns_now();
    if (cur >= ix->cmb_hw || t - ix->cmb_hw_ns > CMB_HW_NS) { ix->cmb_hw = cur; ix->cmb_hw_ns = t; }
}

static int small_combined(tm_index *ix, SmallReq &rq) {
    const uint64_t t_in = g_cmb_timing ? ns_now() : 0;
    struct ReqTime {   // (on every return path)
        uint64_t t;
        ~ReqTime() { if (g_cmb_timing) { g_cmbt.reqs++; g_cmbt.req_ns += ns_now() - t; } }
    } rt{t_in};
    std::unique_lock<std::mutex> lk(ix->cmb_mu);
    ix->cmb_q.push_back(&rq);
    cmb_note_load(ix);
    if (ix->cmb_gathering) ix->cmb_gcv.notify_all();
    while (!rq.done) {
        if (ix->cmb_running < std::max(ix->cmb_leaders.load(), 1) && !ix->cmb_q.empty()) {
            ix->cmb_running++;
            const int gus = ix->cmb_gather_us.load(std::memory_order_relaxed);
            if (gus > 0) {   // the gather window (study knob)
                const auto dl = std::chrono::steady_clock::now() + std::chrono::microseconds(gus);
                ix->cmb_gathering++;
                for (;;) {
                    uint64_t q = 0;
                    for (auto *r : ix->cmb_q) q += r->n;
                    if ((int)ix->cmb_q.size() + ix->cmb_inflight >= ix->cmb_hw || ix->cmb_q.size() >= (size_t)SMALL_SEGS ||
                        q >= ZC_TOPICS)
                        break;
                    if (ix->cmb_gcv.wait_until(lk, dl) == std::cv_status::timeout) break;
                }
                ix->cmb_gathering--;
            }
            std::vector<SmallReq *> grp;
            uint64_t total = 0;
            const bool pairs = ix->cmb_q.front()->pairs;   // a launch carries one output kind: the front's
            for (auto it = ix->cmb_q.begin(); it != ix->cmb_q.end() && grp.size() < (size_t)SMALL_SEGS;) {
                if ((*it)->pairs != pairs || total + (*it)->n > ZC_TOPICS) { ++it; continue; }
                total += (*it)->n;
                grp.push_back(*it);
                it = ix->cmb_q.erase(it);
            }
            ix->cmb_inflight += (int)grp.size();
            if (!ix->cmb_q.empty() && ix->cmb_running < ix->cmb_leaders.load()) ix->cmb_q.front()->cv.notify_one();
            lk.unlock();
            uint64_t t_sync_end = 0;
            const int rc = run_small_group(ix, grp, &t_sync_end);   // (the lane is released on return)
            const uint64_t t_rel = g_cmb_timing ? ns_now() : 0;
            lk.lock();
            if (g_cmb_timing && t_sync_end) {
                g_cmbt.release_ns += t_rel - t_sync_end;
                g_cmbt.done_ns += ns_now() - t_rel;
            }
            for (auto *r : grp) {
                r->rc = rc;
                r->done = true;
                if (r != &rq) { r->poke.store(1, std::memory_order_release); r->cv.notify_one(); }
            }
            ix->cmb_inflight -= (int)grp.size();
            ix->cmb_running--;
            if (!ix->cmb_q.empty()) {   // it may lead now
                ix->cmb_q.front()->poke.store(1, std::memory_order_release);
                ix->cmb_q.front()->cv.notify_one();
            }
            continue;
        }
        const int spin = ix->cmb_spin_us.load(std::memory_order_relaxed);
        if (spin > 0) {   // TM_DEBUG_CMB_SPIN: spin a while before sleeping (no futex wake-up on the reply path)
            rq.poke.store(0, std::memory_order_relaxed);
            lk.unlock();
            const uint64_t dl = ns_now() + (uint64_t)spin * 1000;
            while (!rq.poke.load(std::memory_order_acquire) && ns_now() < dl) __builtin_ia32_pause();
            lk.lock();
            if (rq.done || rq.poke.load(std::memory_order_relaxed)) continue;
        }
        rq.cv.wait(lk);
    }
    return rq.rc;
}

// tm_match_batch_ex, or (to32v) the same over u32 offsets that lie in
// TM_ALLOC_VRAM memory with their bytes (tm_match_batch32_ex's batches the
// one-launch path does not take): widened on the device, never read by the host
// TM_HOST_TIMING=1: its per-phase host timings on stderr (diagnostics)
static int match_batch_impl(tm_index *ix, uint64_t n, const uint8_t *tb, const uint64_t *to, const uint32_t *to32v,
                            uint64_t *out_hit, uint32_t *out_vals, uint64_t cap, uint8_t *out_err, uint32_t order,
                            uint32_t *out_unique) {
    const bool timing = g_cmb_timing;
    const uint64_t t0 = timing ? ns_now() : 0;
    if (n >= 0xFFFFFFFFull) return fail(ix, TM_EINVAL, "tm_match_batch: batch too large");
    if (order > TM_ORDER_UNIQUE) return fail(ix, TM_EINVAL, "tm_match_batch: bad order");
    const bool sorted = order != TM_ORDER_TRAVERSAL, unique = order == TM_ORDER_UNIQUE;
    HostBatch hb(ix);
    int rc;
    if ((rc = hb.open(n))) return rc;
    Lane &ln = *hb.ln;
    const hipStream_t s = ln.s;
    ix->rep[ln.r].batches++;
    const uint64_t t1 = timing ? ns_now() : 0;
    if (n && n <= ZC_TOPICS && !to32v) {
        // every buffer from tm_host_alloc: the kernels read the topics and
        // write the hit lists in place (no staging copy in, no copy out)
        const uint64_t nbytes = to[n];
        bool ok = tb || !nbytes;
        uint8_t *db = opt_dev(ix, tb, nbytes, ok);
        uint8_t *dof = opt_dev(ix, to, (n + 1) * 8, ok);
        uint8_t *dh = opt_dev(ix, out_hit, (n + 1) * 8, ok);
        uint8_t *dv = opt_dev(ix, out_vals, cap * 4, ok);
        uint8_t *de = opt_dev(ix, out_err, n, ok);
        uint8_t *du = opt_dev(ix, out_unique, n * 4, ok);
        const bool aligned = ((uintptr_t)tb & 15) == 0;
        if (ok && aligned) {
            if (!de) {   // flags nobody reads still need a home
                if ((rc = stage_out(ix, ln, n, n, de))) return rc;
            }
            const uint8_t *dbytes = db ? db : dof;   // no bytes: any valid address
            uint64_t *dhit = reinterpret_cast<uint64_t *>(dh);
            uint32_t *vdst = reinterpret_cast<uint32_t *>(dv);
            if (sorted && dv) {   // sorted in HBM, then copied into the caller's buffer
                if ((rc = grow_dev(ix, s, ln.d_vals, ln.d_vals_cap, cap))) return rc;
                vdst = ln.d_vals;
            }
            rc = hb.run([&](const DevIndex &d, uint32_t tag) -> int {
                int path = PATH_PHASES;
                HIPCHK(ix, launch_match(d, ln.w, n, dbytes, reinterpret_cast<const uint64_t *>(dof), dhit, de, vdst,
                                        dv ? cap : 0, tag, next_lb(ix), ix->dbg_phases, ix->small_kind, s, nullptr,
                                        nullptr, &path));
                ix->path_batches[path]++;
                if (sorted && dv) {
                    HIPCHK(ix, launch_sort_segments(ln.w, n, dhit, vdst, cap, unique, reinterpret_cast<uint32_t *>(du), s));
                    HIPCHK(ix, launch_copy_values(dhit, n, vdst, reinterpret_cast<uint32_t *>(dv), cap, s));
                }
                return TM_OK;
            });
            if (rc) return rc;
            if (timing)
                fprintf(stderr, "tm_match_batch n=%lu (in place): sync %.1f launch %.1f wait %.1f us\n",
                        (unsigned long)n, (t1 - t0) * 1e-3, (hb.t_queued - t1) * 1e-3, (hb.t_synced - hb.t_queued) * 1e-3);
            return (out_vals && out_hit[n] > cap) ? TM_ECAP : TM_OK;
        }
    }
    const uint8_t *dbytes;
    const uint64_t *doffs;
    if ((rc = stage_in(ix, ln, n, tb, to, to32v, dbytes, doffs))) return rc;
    const uint64_t t2 = timing ? ns_now() : 0;
    // results: hit offsets (n + 1) x u64, then the badarg flags (then the
    // distinct counts, u32, for UNIQUE); the values are written by k_emit
    // straight into mapped pinned memory (sorted orders: sorted in HBM, then
    // copied there), so the batch costs one host synchronisation (a second
    // one only when that buffer must grow)
    const uint64_t uoff = ((n + 1) * 8 + n + 3) & ~3ull;
    const uint64_t rbytes = (sorted && out_unique) ? uoff + 4 * n : (n + 1) * 8 + n;
    uint8_t *dres;
    if ((rc = stage_out(ix, ln, n, rbytes, dres))) return rc;
    uint64_t *dhit = reinterpret_cast<uint64_t *>(dres);
    uint8_t *derr = dres + (n + 1) * 8;
    uint32_t *dunq = (sorted && out_unique) ? reinterpret_cast<uint32_t *>(dres + uoff) : nullptr;
    uint64_t total = 0;
    for (int attempt = 0;; attempt++) {
        if (!ln.pin_vals) {
            ln.pin_vals_cap = std::max<uint64_t>(ln.pin_vals_cap, 1 << 16);
            HIPCHK(ix, hipHostMalloc(&ln.pin_vals, ln.pin_vals_cap * 4, hipHostMallocMapped));
            HIPCHK(ix, hipHostGetDevicePointer(reinterpret_cast<void **>(&ln.pin_vals_dev), ln.pin_vals, 0));
        }
        if (sorted && (rc = grow_dev(ix, s, ln.d_vals, ln.d_vals_cap, ln.pin_vals_cap))) return rc;
        uint32_t *vdst = sorted ? ln.d_vals : ln.pin_vals_dev;
        rc = hb.run([&](const DevIndex &d, uint32_t tag) -> int {
            int path = PATH_PHASES;
            HIPCHK(ix, launch_match(d, ln.w, n, dbytes, doffs, dhit, derr, vdst, ln.pin_vals_cap, tag, next_lb(ix),
                                    ix->dbg_phases, ix->small_kind, s, nullptr, nullptr, &path));
            ix->path_batches[path]++;
            if (sorted) {
                HIPCHK(ix, launch_sort_segments(ln.w, n, dhit, vdst, ln.pin_vals_cap, unique, dunq, s));
                HIPCHK(ix, launch_copy_values(dhit, n, vdst, ln.pin_vals_dev, ln.pin_vals_cap, s));
            }
            return fetch_out(ix, ln, n, rbytes);
        });
        if (rc) return rc;
        memcpy(&total, ln.pin_out + n * 8, 8);
        if (total <= ln.pin_vals_cap || !out_vals) break;
        if (attempt == 2) return fail(ix, TM_EDEVICE, "tm_match_batch: hit total kept growing past the staging buffer");
        // grow the mapped buffer and run the batch again (rare: sizes are sticky)
        if ((rc = hb.relock())) return rc;
        HIPCHK(ix, hipHostFree(ln.pin_vals));
        ln.pin_vals = nullptr;
        ln.pin_vals_cap = total + total / 4;
    }
    memcpy(out_hit, ln.pin_out, (n + 1) * 8);
    if (out_err && n) memcpy(out_err, ln.pin_out + (n + 1) * 8, n);
    if (dunq && n) memcpy(out_unique, ln.pin_out + uoff, 4 * n);
    const uint64_t keep = std::min(total, out_vals ? cap : 0);
    if (keep) memcpy(out_vals, ln.pin_vals, keep * 4);
    if (timing)
        fprintf(stderr, "tm_match_batch n=%lu: sync %.1f stage %.1f launch %.1f wait %.1f copy-out %.1f us\n",
                (unsigned long)n, (t1 - t0) * 1e-3, (t2 - t1) * 1e-3, (hb.t_queued - t2) * 1e-3,
                (hb.t_synced - hb.t_queued) * 1e-3, (ns_now() - hb.t_synced) * 1e-3);
    return (out_vals && total > cap) ? TM_ECAP : TM_OK;
}

int tm_match_batch_ex(tm_index *ix, uint64_t n, const uint8_t *tb, const uint64_t *to, uint64_t *out_hit,
                      uint32_t *out_vals, uint64_t cap, uint8_t *out_err, uint32_t order, uint32_t *out_unique) {
    if (!ix) return fail(nullptr, TM_EINVAL, "tm_match_batch: null handle");
    if (!to || !out_hit || (n && !tb && to[n] != to[0])) return fail(ix, TM_EINVAL, "tm_match_batch: null buffer");
    return match_batch_impl(ix, n, tb, to, nullptr, out_hit, out_vals, cap, out_err, order, out_unique);
}

int tm_match_batch(tm_index *ix, uint64_t n, const uint8_t *tb, const uint64_t *to, uint64_t *out_hit,
                   uint32_t *out_vals, uint64_t cap, uint8_t *out_err) {
    return tm_match_batch_ex(ix, n, tb, to, out_hit, out_vals, cap, out_err, TM_ORDER_TRAVERSAL, nullptr);
}

// ---- the route fan-out on a host lane's scratch (tm_route_batch, and the
// batches of tm_route_batch32 that k_fo_one does not take)

// room for vcap entries over n_dests destinations: the fan-out's arrays and
// passes (pairs: from the n topics' spans), and under aggre the kept ones
static int route_scratch(tm_index *ix, Lane &ln, uint32_t n_dests, uint64_t vcap, bool aggre, bool pairs, uint64_t n) {
    int rc;
    const hipStream_t s = ln.s;
    if ((rc = grow_dev(ix, s, ln.d_ft, ln.d_ft_cap, vcap))) return rc;
    if ((rc = grow_dev(ix, s, ln.d_fv, ln.d_fv_cap, vcap))) return rc;
    if ((rc = grow_dev(ix, s, ln.d_fo, ln.d_fo_cap, (uint64_t)n_dests + 2))) return rc;
    if ((rc = ensure_fanout(ix, ln, n_dests, vcap, pairs, n))) return rc;
    if (!aggre) return TM_OK;
    if ((rc = grow_dev(ix, s, ln.d_at, ln.d_at_cap, vcap))) return rc;
    if ((rc = grow_dev(ix, s, ln.d_av, ln.d_av_cap, vcap))) return rc;
    if ((rc = grow_dev(ix, s, ln.d_ao, ln.d_ao_cap, (uint64_t)n_dests + 2))) return rc;
    return ensure_aggre(ix, ln, vcap);
}

// queues the grid fan-out of the lane's matched values (d_vals; their CSR
// offsets `hit`, or with `pairs` their spans) into d_fo/d_ft/d_fv with the
// index's own destination table, and with `aggre` the aggre pass over that
// into d_ao/d_at/d_av (caller holds ix->mu)
static int queue_grid_fanout(tm_index *ix, Lane &ln, uint64_t n, const uint64_t *hit, const uint32_t *pairs,
                             uint64_t vcap, uint32_t n_dests, bool aggre) {
    int rc;
    const hipStream_t s = ln.s;
    const int grp = ix->rep[ln.r].group;
    const uint32_t *dtab = nullptr, *ftab = nullptr;
    uint64_t dlen = 0, flen = 0;
    if ((rc = dest_upload(ix, grp, s, dtab, dlen))) return rc;
    uint32_t *ft = ln.d_ft, *fv = ln.d_fv;
    if (pairs) HIPCHK(ix, launch_fanout_pairs(ln.f, n, pairs, ln.d_vals, vcap, dtab, dlen, n_dests, ln.d_fo, ft, fv, s));
    else HIPCHK(ix, launch_fanout(ln.f, n, hit, ln.d_vals, vcap, dtab, dlen, n_dests, ln.d_fo, ft, fv, s));
    if (!aggre) return TM_OK;
    if ((rc = filter_upload(ix, grp, s, ftab, flen))) return rc;
    HIPCHK(ix, launch_aggre(ln.f, n_dests, ln.d_fo, ln.d_ft, ln.d_fv, vcap, ftab, flen, ln.d_ao, ln.d_at, ln.d_av, s));
    return TM_OK;
}

// tm_dispatch_batch's dispatch half: which bucket, the caller's outputs, and
// where on the device the head words land (with the batch's results)
struct RouteDispatch {
    uint32_t local_dest;
    uint64_t *out_head;
    uint32_t *out_topic, *out_value, *out_sub;
    uint64_t dcap;
};

// queues the dispatch of bucket `bucket` of the lane's fan-out results (d_fo /
// d_ft / d_fv, under aggre d_ao / d_at / d_av) with the index's own subscriber
// table into d_dt / d_dv / d_ds, at most out_cap deliveries; head = [M, T]
// (caller holds ix->mu).  queue_dispatch_to: the bucket offsets and the outputs
// as given (tm_dispatch_batch32: the caller's own buffers).
static int queue_dispatch_to(tm_index *ix, Lane &ln, uint32_t n_dests, uint32_t bucket, const uint64_t *doff,
                             bool aggre, uint64_t vcap, uint64_t out_cap, uint64_t *d_head, uint32_t *dt, uint32_t *dv,
                             uint32_t *ds) {
    int rc;
    const hipStream_t s = ln.s;
    const uint32_t *span = nullptr, *pool = nullptr;
    uint64_t span_len = 0, pool_len = 0;
    if ((rc = subs_upload(ix, ix->rep[ln.r].group, s, span, span_len, pool, pool_len))) return rc;
    HIPCHK(ix, launch_dispatch(ln.f, n_dests, doff, bucket, aggre ? ln.d_at : ln.d_ft, aggre ? ln.d_av : ln.d_fv, vcap,
                               span, span_len, pool, pool_len, d_head, nullptr, dt, dv, ds, out_cap, s));
    return TM_OK;
}

static int queue_dispatch(tm_index *ix, Lane &ln, uint32_t n_dests, uint32_t bucket, bool aggre, uint64_t vcap,
                          uint64_t out_cap, uint64_t *d_head) {
    return queue_dispatch_to(ix, ln, n_dests, bucket, aggre ? ln.d_ao : ln.d_fo, aggre, vcap, out_cap, d_head, ln.d_dt,
                             ln.d_dv, ln.d_ds);
}

// room for `want` deliveries on the lane
static int dispatch_scratch(tm_index *ix, Lane &ln, uint64_t vcap, uint64_t want) {
    int rc;
    if ((rc = ensure_dispatch(ix, ln, vcap, true))) return rc;
    if ((rc = grow_dev(ix, ln.s, ln.d_dt, ln.d_dt_cap, want))) return rc;
    if ((rc = grow_dev(ix, ln.s, ln.d_dv, ln.d_dv_cap, want))) return rc;
    return grow_dev(ix, ln.s, ln.d_ds, ln.d_ds_cap, want);
}

// tm_deliver_batch's grouping half: the caller's group outputs (the three
// delivery arrays of the dispatch half arrive grouped)
struct RouteGroup {
    uint64_t *out_ghead;
    uint32_t *out_gsub;
    uint64_t *out_goff;
    uint64_t gcap;
    uint32_t *out_goff32 = nullptr;   // tm_deliver_batch32: the caller's offsets, narrowed on the way out (out_goff null)
};

// room on the lane for `want` grouped deliveries and min(gcap, want) groups
// (G <= W <= want: a lane array that is short means the caller's is)
static int group_scratch(tm_index *ix, Lane &ln, uint64_t want, uint64_t gcap, const char *who) {
    int rc;
    const uint64_t groom = std::min(gcap, want);
    if ((rc = ensure_group(ix, ln, want, who))) return rc;
    if ((rc = grow_dev(ix, ln.s, ln.d_gt, ln.d_gt_cap, want))) return rc;
    if ((rc = grow_dev(ix, ln.s, ln.d_gv, ln.d_gv_cap, want))) return rc;
    if ((rc = grow_dev(ix, ln.s, ln.d_gs, ln.d_gs_cap, want))) return rc;
    if ((rc = grow_dev(ix, ln.s, ln.d_gsub, ln.d_gsub_cap, groom))) return rc;
    return grow_dev(ix, ln.s, ln.d_goff, ln.d_goff_cap, groom + 1);
}

// queues the grouping of the lane's deliveries (d_dt / d_dv / d_ds, the first
// min(d_head[1], out_cap) of them: what queue_dispatch was given) into d_gt /
// d_gv / d_gs, d_gsub and d_goff; d_ghead = [G, W] (caller holds ix->mu)
static int queue_group(tm_index *ix, Lane &ln, const uint64_t *d_head, uint64_t out_cap, uint64_t gcap,
                       uint64_t *d_ghead) {
    HIPCHK(ix, launch_group_subs(ln.f, d_head, ln.d_dt, ln.d_dv, ln.d_ds, out_cap, d_ghead, ln.d_gsub, ln.d_goff,
                                 std::min(gcap, out_cap), ln.d_gt, ln.d_gv, ln.d_gs, nullptr, ln.s));
    return TM_OK;
}

// tm_publish_batch's pick half: the per-topic key words (host, n each, may be
// null), the seed, and the caller's member array (aligned with out_topic)
struct RoutePick {
    const uint32_t *key_clientid, *key_topic;
    uint32_t seed;
    uint32_t *out_member;
};

// queues the shared-subscription pick over the lane's aggregated results (d_ao
// / d_at / d_av) with the index's own tables and state into d_sm (caller
// holds ix->mu).  Queued ONCE per call, after the run that stands: the state
// words move once, and only for entries the caller gets.
static int queue_pick(tm_index *ix, Lane &ln, uint64_t n, uint32_t n_dests, uint64_t vcap, const RoutePick &pk,
                      const uint64_t *doff = nullptr) {
    int rc;
    const hipStream_t s = ln.s;
    const uint64_t hoff = (vcap + 1) & ~1ull;   // the two head words, 8-byte aligned
    if ((rc = ensure_share(ix, ln, vcap))) return rc;
    if ((rc = grow_dev(ix, s, ln.d_sm, ln.d_sm_cap, hoff + 4))) return rc;
    const uint32_t *kc = nullptr, *kt = nullptr;
    if (n && (pk.key_clientid || pk.key_topic)) {
        if ((rc = grow_dev(ix, s, ln.d_sk, ln.d_sk_cap, 2 * n))) return rc;
        if (pk.key_clientid) {
            HIPCHK(ix, hipMemcpyAsync(ln.d_sk, pk.key_clientid, n * 4, hipMemcpyHostToDevice, s));
            kc = ln.d_sk;
        }
        if (pk.key_topic) {
            HIPCHK(ix, hipMemcpyAsync(ln.d_sk + n, pk.key_topic, n * 4, hipMemcpyHostToDevice, s));
            kt = ln.d_sk + n;
        }
    }
    const uint32_t *slot_of = nullptr, *rec = nullptr, *pool = nullptr;
    uint64_t slot_len = 0, n_slots = 0, pool_len = 0;
    uint32_t *state = nullptr;
    if ((rc = share_upload(ix, ix->rep[ln.r].group, s, slot_of, slot_len, rec, n_slots, pool, pool_len, state))) return rc;
    HIPCHK(ix, launch_share_pick(ln.f, n_dests, doff ? doff : ln.d_ao, ln.d_at, ln.d_av, vcap, kc, kt, n, pk.seed, slot_of, slot_len, rec,
                                 n_slots, pool, pool_len, state, reinterpret_cast<uint64_t *>(ln.d_sm + hoff), ln.d_sm, s));
    return TM_OK;
}

// The lane's fan-out results to the caller (the lock is not held; the lane is
// still checked out: its buffers are this caller's).  `fo`: n_dests + 2 u64
// the offsets land in -- the caller's own array, or narrowed into fo32.
// aggre_ran: the aggre pass's offsets, then its kept entries (two waits: the
// count comes with the offsets).  Otherwise the fan-out's offsets and the
// first min(total, cap) entries -- none under aggre, which then had no room
// (TM_ECAP: the un-aggregated sizes).
static int copy_route_out(tm_index *ix, Lane &ln, uint32_t n_dests, uint64_t total, uint64_t cap, bool aggre,
                          bool aggre_ran, uint64_t *fo, uint32_t *fo32, uint32_t *out_topic, uint32_t *out_values) {
    const hipStream_t s = ln.s;
    const uint64_t nfo = (uint64_t)n_dests + 2;
    if (aggre_ran) {
        HIPCHK(ix, hipMemcpyAsync(fo, ln.d_ao, nfo * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(ix, hipStreamSynchronize(s));
        const uint64_t kept = std::min(fo[n_dests + 1], cap);   // (K <= total <= cap)
        if (kept) {
            HIPCHK(ix, hipMemcpyAsync(out_topic, ln.d_at, kept * 4, hipMemcpyDeviceToHost, s));
            HIPCHK(ix, hipMemcpyAsync(out_values, ln.d_av, kept * 4, hipMemcpyDeviceToHost, s));
            HIPCHK(ix, hipStreamSynchronize(s));
        }
    } else {
        const uint64_t keep = aggre ? 0 : std::min(total, cap);
        HIPCHK(ix, hipMemcpyAsync(fo, ln.d_fo, nfo * 8, hipMemcpyDeviceToHost, s));
        if (keep) {
            HIPCHK(ix, hipMemcpyAsync(out_topic, ln.d_ft, keep * 4, hipMemcpyDeviceToHost, s));
            HIPCHK(ix, hipMemcpyAsync(out_values, ln.d_fv, keep * 4, hipMemcpyDeviceToHost, s));
        }
        HIPCHK(ix, hipStreamSynchronize(s));
    }
    if (fo32)
        for (uint64_t i = 0; i < nfo; i++) fo32[i] = (uint32_t)fo[i];
    return total > cap ? TM_ECAP : TM_OK;
}

// One request of the route family (tm_route_batch, tm_dispatch_batch,
// tm_publish_batch and their 32-bit forms): everything the six entry points
// share.  dp / pk / gp: the dispatch, the pick and the grouping of the
// deliveries (tm_deliver_batch; with dp only), null when the call has none;
// pk and gp together: tm_publish_deliver_batch, the local picks merged in.
// who: the entry point the caller called -- every refusal and failure names
// it.  Only the topic offsets and out_dest_offsets differ in width; they travel
// beside the request.
struct RouteReq {
    const char *who;
    uint64_t n;
    const uint8_t *tb;
    uint32_t n_dests, flags;
    uint32_t *out_topic, *out_values;
    uint64_t cap;
    uint8_t *out_err;
    const RouteDispatch *dp;
    const RoutePick *pk;
    const RouteGroup *gp = nullptr;
    bool aggre() const { return flags & TM_ROUTE_AGGRE; }
};

static int route_fail(tm_index *ix, const RouteReq &rq, int code, const char *what) {
    return fail(ix, code, std::string(rq.who) + ": " + what);
}

// What a grouping left on the lane (d_gt / d_gv / d_gs, d_gsub, d_goff), to
// the caller (the lock is not held; the lane is still checked out): head = [M,
// T, G, W] as the device left it, the first min(T, dcap) grouped deliveries,
// the first min(G, gcap) subscribers, and their offsets with the end entry --
// into out_goff, or narrowed into out_goff32 (tm_deliver_batch32) through a
// per-thread buffer of min(G, gcap) + 1 words: sized from G, never from the
// caller's capacities.  The caller's arrays are pageable memory or
// tm_host_alloc buffers.
static int copy_group_out(tm_index *ix, Lane &ln, const RouteReq &rq, const uint64_t head[4]) {
    const hipStream_t s = ln.s;
    const RouteDispatch *dp = rq.dp;
    const RouteGroup *gp = rq.gp;
    const uint64_t dcap = std::min<uint64_t>(dp->dcap, 0xFFFFFFFFull);
    // (behind a pick the grouped arrays hold the N = head[3] merged deliveries)
    const uint64_t keep = std::min(rq.pk ? head[3] : head[1], dcap), gkeep = std::min(head[2], gp->gcap);
    static thread_local std::vector<uint64_t> wide;
    uint64_t *goff = gp->out_goff;
    if (!goff) {
        try {
            wide.resize(gkeep + 1);
        } catch (const std::bad_alloc &) {
            return route_fail(ix, rq, TM_ENOMEM, "out of host memory");
        }
        goff = wide.data();
    }
    dp->out_head[0] = head[0];
    dp->out_head[1] = head[1];
    gp->out_ghead[0] = head[2];
    gp->out_ghead[1] = head[3];
    if (keep) {
        HIPCHK(ix, hipMemcpyAsync(dp->out_topic, ln.d_gt, keep * 4, hipMemcpyDefault, s));
        HIPCHK(ix, hipMemcpyAsync(dp->out_value, ln.d_gv, keep * 4, hipMemcpyDefault, s));
        HIPCHK(ix, hipMemcpyAsync(dp->out_sub, ln.d_gs, keep * 4, hipMemcpyDefault, s));
    }
    if (gkeep) HIPCHK(ix, hipMemcpyAsync(gp->out_gsub, ln.d_gsub, gkeep * 4, hipMemcpyDefault, s));
    HIPCHK(ix, hipMemcpyAsync(goff, ln.d_goff, (gkeep + 1) * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(ix, hipStreamSynchronize(s));
    if (!gp->out_goff)
        for (uint64_t i = 0; i <= gkeep; i++) gp->out_goff32[i] = (uint32_t)goff[i];
    return TM_OK;
}

// The family's argument checks, once per call, before anything is locked or
// queued.  offsets: the topic offsets and out_dest_offsets are both there.
// narrow: a 32-bit call, which may run in place -- out_err is required (the
// device writes the flags there) and so is an out_head the device can write
// as two u64.
static int route_check(tm_index *ix, const RouteReq &rq, bool offsets, bool narrow) {
    const RouteDispatch *dp = rq.dp;
    if (!ix) return route_fail(nullptr, rq, TM_EINVAL, "null handle");
    if (rq.flags & ~(uint32_t)TM_ROUTE_AGGRE) return route_fail(ix, rq, TM_EINVAL, "unknown flag");
    if (rq.pk && !rq.aggre())
        return route_fail(ix, rq, TM_EINVAL, "TM_ROUTE_AGGRE is required (aggre/1 runs before route/2)");
    if (!rq.n_dests || rq.n_dests > FO_MAX_DESTS) return route_fail(ix, rq, TM_EINVAL, "n_dests must be 1 .. 65536");
    if (dp && dp->local_dest >= rq.n_dests) return route_fail(ix, rq, TM_EINVAL, "local_dest must be below n_dests");
    if (!offsets || (narrow && !rq.out_err) ||
        (rq.cap && (!rq.out_topic || !rq.out_values || (rq.pk && !rq.pk->out_member))) ||
        (dp && (!dp->out_head || (dp->dcap && (!dp->out_topic || !dp->out_value || !dp->out_sub)))))
        return route_fail(ix, rq, TM_EINVAL, "null buffer");
    if (rq.gp && (!dp || !rq.gp->out_ghead || !(narrow ? (const void *)rq.gp->out_goff32 : (const void *)rq.gp->out_goff) ||
                  (rq.gp->gcap && !rq.gp->out_gsub)))
        return route_fail(ix, rq, TM_EINVAL, "null buffer");
    if (narrow && dp && ((uintptr_t)dp->out_head & 7)) return route_fail(ix, rq, TM_EINVAL, "out_head must be 8-byte aligned");
    if (narrow && rq.gp && ((uintptr_t)rq.gp->out_ghead & 7))
        return route_fail(ix, rq, TM_EINVAL, "out_ghead must be 8-byte aligned");
    if (rq.n >= 0xFFFFFFFFull) return route_fail(ix, rq, TM_EINVAL, "batch too large");
    return TM_OK;
}

// The pick of a call whose run stands (no scratch grows, no retry is left) and
// whose caller has the `kept` entries: queued now, ONCE, over the arrays still
// in the lane -- the state words move once, and only for entries the caller
// gets.  Only the copy of its own output can fail after it.
// gm (tm_publish_deliver_batch): behind the pick, in the same hold of the lock
// and on the same lane, the picks are merged with the lane's gm->T deliveries
// (d_head = [M, T] on the device) and grouped into the lane's group arrays,
// d_head[2..3] = [G, N]; gm->fetch: d_head is not mapped host memory, its four
// words are copied to gm->pin.  Every scratch is had BEFORE the pick is queued:
// a call that runs out of memory has moved no state.
struct PickMerge {
    uint64_t *d_head, T, gcap;
    uint8_t *pin;
    bool fetch;
    const uint64_t *doff = nullptr;   // the aggre pass's offsets where they are not ln.d_ao (u32 there, widened here)
    bool locked = false;              // the caller holds the lock and has queued on the lane in this hold
};

static int pick_after_run(tm_index *ix, HostBatch &hb, const RouteReq &rq, uint64_t vcap, uint64_t kept,
                          const PickMerge *gm = nullptr) {
    int rc;
    Lane &ln = *hb.ln;
    if (!(gm && gm->locked) && (rc = hb.relock())) return rc;
    const uint32_t *sub_of = nullptr;
    uint64_t sub_of_len = 0;
    // (a topic index is below n: the digits the picks' sort by message can need)
    const uint32_t msg_passes = rq.n <= 0x100 ? 1 : rq.n <= 0x10000 ? 2 : rq.n <= 0x1000000 ? 3 : GS_PASSES;
    if (gm) {
        if ((rc = group_scratch(ix, ln, gm->T + kept, gm->gcap, rq.who))) return rc;
        if ((rc = ensure_group_picks(ix, ln, gm->T + kept, kept, rq.who))) return rc;
        if ((rc = msub_upload(ix, ix->rep[ln.r].group, ln.s, sub_of, sub_of_len))) return rc;
    }
    if ((rc = queue_pick(ix, ln, rq.n, rq.n_dests, vcap, *rq.pk, gm ? gm->doff : nullptr))) return rc;
    if (gm) {
        HIPCHK(ix, launch_group_picks(ln.f, gm->d_head, ln.d_dt, ln.d_dv, ln.d_ds, gm->T, rq.n_dests,
                                      gm->doff ? gm->doff : ln.d_ao, ln.d_at,
                                      ln.d_av, ln.d_sm, kept, sub_of, sub_of_len, gm->d_head + 2, ln.d_gsub, ln.d_goff,
                                      std::min(gm->gcap, gm->T + kept), ln.d_gt, ln.d_gv, ln.d_gs, nullptr,
                                      gm->T + kept, msg_passes, ln.s));
        if (gm->fetch) HIPCHK(ix, hipMemcpyAsync(gm->pin, gm->d_head, 32, hipMemcpyDeviceToHost, ln.s));
    }
    if ((rc = batch_done(ix, ln))) return rc;
    hb.g.unlock();
    // (the copy may wait for the stream: never under the lock.  out_member is
    // pageable memory or, after a 32-bit call, a tm_host_alloc buffer)
    if (kept) HIPCHK(ix, hipMemcpyAsync(rq.pk->out_member, ln.d_sm, kept * 4, hipMemcpyDefault, ln.s));
    HIPCHK(ix, hipStreamSynchronize(ln.s));
    return TM_OK;
}

// The product path of a batched broker (the request already checked): match
// into device scratch (CSR, traversal order), fan out with the index's own
// destination table, copy the destination-major arrays back.  The lane's value
// scratch always holds the whole batch (it grows and the batch runs again), so
// the bucket offsets are complete whatever `cap` is; cap only bounds what is
// copied out.
// TM_ROUTE_AGGRE: the aggre pass runs on the fan-out's results in the lane's
// scratch, and only the kept entries are copied back.
// dp (tm_dispatch_batch): in the same run, on the same lane, the dispatch of
// bucket dp->local_dest over the results; the lane's delivery scratch grows
// from the T that comes back with the results, and then only the dispatch
// kernels are queued again.
// gp (tm_deliver_batch): behind every dispatch queued, on the same lane, the
// grouping of its deliveries; the copies out read the grouped arrays.  The
// lane's group arrays hold min(gcap, deliveries) groups, so nothing but the
// dispatch's own retry ever queues it again.
// pk (tm_publish_batch): pick_after_run, when the kept entries fit.
// pk and gp (tm_publish_deliver_batch): the run queues no grouping; when the
// kept entries fit and T + K <= dcap (both known here, K bounds the local
// picks), pick_after_run queues the pick and behind it the merge of the local
// picks with the lane's deliveries and their grouping, and the copies out read
// the merged arrays.  Otherwise TM_ECAP with no pick made and no state moved.
static int route_batch_impl(tm_index *ix, const RouteReq &rq, const uint64_t *to, uint64_t *out_dest_offsets) {
    const uint64_t n = rq.n, cap = rq.cap;
    const uint32_t n_dests = rq.n_dests;
    const bool aggre = rq.aggre();
    const RouteDispatch *dp = rq.dp;
    const RouteGroup *gp = rq.gp;
    const bool merge = gp && rq.pk;   // tm_publish_deliver_batch: the grouping waits for the pick
    HostBatch hb(ix, rq.who);
    int rc;
    if ((rc = hb.open(n))) return rc;
    Lane &ln = *hb.ln;
    const hipStream_t s = ln.s;
    ix->rep[ln.r].batches++;
    const uint8_t *dbytes;
    const uint64_t *doffs;
    if ((rc = stage_in(ix, ln, n, rq.tb, to, nullptr, dbytes, doffs))) return rc;
    // hit offsets, then the err flags; with a dispatch its two head words after them, then the grouping's
    const uint64_t hoff = ((n + 1) * 8 + n + 7) & ~7ull;
    const uint64_t hbytes = gp ? 32 : 16;
    const uint64_t rbytes = dp ? hoff + hbytes : (n + 1) * 8 + n;
    uint8_t *dres;
    if ((rc = stage_out(ix, ln, n, rbytes, dres))) return rc;
    uint64_t *dhit = reinterpret_cast<uint64_t *>(dres);
    uint8_t *derr = dres + (n + 1) * 8;
    uint64_t *dhead = reinterpret_cast<uint64_t *>(dres + hoff);
    const uint64_t gcap = gp ? gp->gcap : 0;
    const uint64_t dcap = dp ? std::min<uint64_t>(dp->dcap, 0xFFFFFFFFull) : 0;
    uint64_t total = 0, vcap = std::max<uint64_t>({ln.d_vals_cap, 4 * n, 1 << 16});
    uint64_t dwant = dp ? std::max<uint64_t>(ln.d_ds_cap, 1 << 16) : 0;   // deliveries the lane has room for
    for (int attempt = 0;; attempt++) {
        if (vcap > 0xFFFFFFFFull) return route_fail(ix, rq, TM_EINVAL, "more than 2^32 - 1 hits in one batch");
        if ((rc = grow_dev(ix, s, ln.d_vals, ln.d_vals_cap, vcap))) return rc;
        if ((rc = route_scratch(ix, ln, n_dests, vcap, aggre, false, 0))) return rc;
        if (dp && (rc = dispatch_scratch(ix, ln, vcap, dwant))) return rc;
        if (gp && !merge && (rc = group_scratch(ix, ln, dwant, gcap, rq.who))) return rc;
        rc = hb.run([&](const DevIndex &d, uint32_t tag) -> int {
            int path = PATH_PHASES;
            HIPCHK(ix, launch_match(d, ln.w, n, dbytes, doffs, dhit, derr, ln.d_vals, vcap, tag, next_lb(ix),
                                    ix->dbg_phases, ix->small_kind, s, nullptr, nullptr, &path));
            ix->path_batches[path]++;
            // (aggre before the total is known: no second wait when it fits)
            if (int rc = queue_grid_fanout(ix, ln, n, dhit, nullptr, vcap, n_dests, aggre)) return rc;
            if (dp)
                if (int rc = queue_dispatch(ix, ln, n_dests, dp->local_dest, aggre, vcap, std::min(dwant, dcap), dhead))
                    return rc;
            if (gp && !merge)
                if (int rc = queue_group(ix, ln, dhead, std::min(dwant, dcap), gcap, dhead + 2)) return rc;
            return fetch_out(ix, ln, n, rbytes);
        });
        if (rc) return rc;
        std::memcpy(&total, ln.pin_out + n * 8, 8);
        if (total <= vcap) break;
        if (attempt >= 2) return route_fail(ix, rq, TM_EDEVICE, "hit total kept growing past the value scratch");
        vcap = total + total / 4;
        if ((rc = hb.relock())) return rc;
    }
    uint64_t head[4] = {0, 0, 0, 0};   // [M, T], then the grouping's [G, W]
    if (dp) {
        std::memcpy(head, ln.pin_out + hoff, hbytes);
        for (int attempt = 0; std::min(head[1], dcap) > dwant; attempt++) {
            // more deliveries than the lane had room for: the scratch grows and the
            // dispatch alone runs again on the results still in the lane (no walk)
            if (attempt >= 2) return route_fail(ix, rq, TM_EDEVICE, "the delivery total kept growing past the scratch");
            dwant = std::min(head[1] + head[1] / 4, dcap);
            if ((rc = hb.relock())) return rc;
            if ((rc = dispatch_scratch(ix, ln, vcap, dwant))) return rc;
            if (gp && !merge && (rc = group_scratch(ix, ln, dwant, gcap, rq.who))) return rc;
            if ((rc = queue_dispatch(ix, ln, n_dests, dp->local_dest, aggre, vcap, dwant, dhead))) return rc;
            if (gp && !merge && (rc = queue_group(ix, ln, dhead, dwant, gcap, dhead + 2))) return rc;
            if (n > ZC_TOPICS) HIPCHK(ix, hipMemcpyAsync(ln.pin_out + hoff, dhead, hbytes, hipMemcpyDeviceToHost, s));
            if ((rc = batch_done(ix, ln))) return rc;
            hb.g.unlock();
            HIPCHK(ix, hipStreamSynchronize(s));
            std::memcpy(head, ln.pin_out + hoff, hbytes);
        }
    }
    rc = copy_route_out(ix, ln, n_dests, total, cap, aggre, aggre && total <= cap, out_dest_offsets, nullptr, rq.out_topic,
                        rq.out_values);
    if (rc != TM_OK && rc != TM_ECAP) return rc;
    if (rq.out_err && n) std::memcpy(rq.out_err, ln.pin_out + (n + 1) * 8, n);
    if (merge) {
        // no pick unless the caller gets every entry and every merged delivery: K bounds the local picks
        const uint64_t kept = rc == TM_OK ? std::min(out_dest_offsets[n_dests + 1], cap) : 0;
        dp->out_head[0] = head[0];
        dp->out_head[1] = head[1];
        gp->out_ghead[0] = gp->out_ghead[1] = 0;
        if (rc != TM_OK || head[1] + kept > dp->dcap || head[1] + kept > 0xFFFFFFFFull) return TM_ECAP;
        const PickMerge gm{dhead, head[1], gcap, ln.pin_out + hoff, n > ZC_TOPICS};
        if (int prc = pick_after_run(ix, hb, rq, vcap, kept, &gm)) return prc;
        std::memcpy(head, ln.pin_out + hoff, hbytes);
        if (int grc = copy_group_out(ix, ln, rq, head)) return grc;
        return head[2] > gcap ? TM_ECAP : TM_OK;
    }
    if (rq.pk && aggre && total <= cap)
        if (int prc = pick_after_run(ix, hb, rq, vcap, std::min(out_dest_offsets[n_dests + 1], cap))) return prc;
    if (gp) {
        if (int grc = copy_group_out(ix, ln, rq, head)) return grc;
        if (head[1] > dp->dcap || head[2] > gcap) rc = TM_ECAP;
    } else if (dp) {
        dp->out_head[0] = head[0];
        dp->out_head[1] = head[1];
        const uint64_t keep = std::min(head[1], dcap);
        if (keep) {
            HIPCHK(ix, hipMemcpyAsync(dp->out_topic, ln.d_dt, keep * 4, hipMemcpyDeviceToHost, s));
            HIPCHK(ix, hipMemcpyAsync(dp->out_value, ln.d_dv, keep * 4, hipMemcpyDeviceToHost, s));
            HIPCHK(ix, hipMemcpyAsync(dp->out_sub, ln.d_ds, keep * 4, hipMemcpyDeviceToHost, s));
            HIPCHK(ix, hipStreamSynchronize(s));
        }
        if (head[1] > dp->dcap) rc = TM_ECAP;
    }
    return rc;
}

// the 64-bit entry points: checked, then route_batch_impl
static int route_batch64(tm_index *ix, const RouteReq &rq, const uint64_t *to, uint64_t *out_dest_offsets) {
    if (int rc = route_check(ix, rq, to && out_dest_offsets, false)) return rc;
    if (rq.n && !rq.tb && to[rq.n] != to[0]) return route_fail(ix, rq, TM_EINVAL, "null buffer");
    return route_batch_impl(ix, rq, to, out_dest_offsets);
}

int tm_route_batch_ex(tm_index *ix, uint64_t n, const uint8_t *tb, const uint64_t *to, uint32_t n_dests,
                      uint64_t *out_dest_offsets, uint32_t *out_topic, uint32_t *out_values, uint64_t cap,
                      uint8_t *out_err, uint32_t flags) {
    const RouteReq rq{"tm_route_batch_ex", n, tb, n_dests, flags, out_topic, out_values, cap, out_err, nullptr, nullptr};
    return route_batch64(ix, rq, to, out_dest_offsets);
}

int tm_route_batch(tm_index *ix, uint64_t n, const uint8_t *tb, const uint64_t *to, uint32_t n_dests,
                   uint64_t *out_dest_offsets, uint32_t *out_topic, uint32_t *out_values, uint64_t cap,
                   uint8_t *out_err) {
    const RouteReq rq{"tm_route_batch", n, tb, n_dests, 0, out_topic, out_values, cap, out_err, nullptr, nullptr};
    return route_batch64(ix, rq, to, out_dest_offsets);
}

int tm_dispatch_batch(tm_index *ix, uint64_t n, const uint8_t *tb, const uint64_t *to, uint32_t n_dests,
                      uint32_t local_dest, uint32_t flags, uint64_t *out_dest_offsets, uint32_t *out_topic,
                      uint32_t *out_values, uint64_t cap, uint64_t *out_head, uint32_t *out_dtopic, uint32_t *out_dvalue,
                      uint32_t *out_dsub, uint64_t dcap, uint8_t *out_err) {
    const RouteDispatch dp{local_dest, out_head, out_dtopic, out_dvalue, out_dsub, dcap};
    const RouteReq rq{"tm_dispatch_batch", n, tb, n_dests, flags, out_topic, out_values, cap, out_err, &dp, nullptr};
    return route_batch64(ix, rq, to, out_dest_offsets);
}

int tm_deliver_batch(tm_index *ix, uint64_t n, const uint8_t *tb, const uint64_t *to, uint32_t n_dests,
                     uint32_t local_dest, uint32_t flags, uint64_t *out_dest_offsets, uint32_t *out_topic,
                     uint32_t *out_values, uint64_t cap, uint64_t *out_head, uint32_t *out_dtopic, uint32_t *out_dvalue,
                     uint32_t *out_dsub, uint64_t dcap, uint64_t *out_ghead, uint32_t *out_gsub, uint64_t *out_goff,
                     uint64_t gcap, uint8_t *out_err) {
    const RouteDispatch dp{local_dest, out_head, out_dtopic, out_dvalue, out_dsub, dcap};
    const RouteGroup gp{out_ghead, out_gsub, out_goff, gcap};
    const RouteReq rq{"tm_deliver_batch", n, tb, n_dests, flags, out_topic, out_values, cap, out_err, &dp, nullptr, &gp};
    return route_batch64(ix, rq, to, out_dest_offsets);
}

int tm_publish_batch(tm_index *ix, uint64_t n, const uint8_t *tb, const uint64_t *to, uint32_t n_dests,
                     uint32_t local_dest, uint32_t flags, uint64_t *out_dest_offsets, uint32_t *out_topic,
                     uint32_t *out_values, uint64_t cap, uint64_t *out_head, uint32_t *out_dtopic, uint32_t *out_dvalue,
                     uint32_t *out_dsub, uint64_t dcap, const uint32_t *key_clientid, const uint32_t *key_topic,
                     uint32_t seed, uint32_t *out_member, uint8_t *out_err) {
    const RouteDispatch dp{local_dest, out_head, out_dtopic, out_dvalue, out_dsub, dcap};
    const RoutePick pk{key_clientid, key_topic, seed, out_member};
    const RouteReq rq{"tm_publish_batch", n, tb, n_dests, flags, out_topic, out_values, cap, out_err, &dp, &pk};
    return route_batch64(ix, rq, to, out_dest_offsets);
}

int tm_publish_deliver_batch(tm_index *ix, uint64_t n, const uint8_t *tb, const uint64_t *to, uint32_t n_dests,
                             uint32_t local_dest, uint32_t flags, uint64_t *out_dest_offsets, uint32_t *out_topic,
                             uint32_t *out_values, uint64_t cap, uint64_t *out_head, uint32_t *out_dtopic,
                             uint32_t *out_dvalue, uint32_t *out_dsub, uint64_t dcap, const uint32_t *key_clientid,
                             const uint32_t *key_topic, uint32_t seed, uint32_t *out_member, uint64_t *out_ghead,
                             uint32_t *out_gsub, uint64_t *out_goff, uint64_t gcap, uint8_t *out_err) {
    const RouteDispatch dp{local_dest, out_head, out_dtopic, out_dvalue, out_dsub, dcap};
    const RoutePick pk{key_clientid, key_topic, seed, out_member};
    const RouteGroup gp{out_ghead, out_gsub, out_goff, gcap};
    const RouteReq rq{"tm_publish_deliver_batch", n, tb, n_dests, flags, out_topic, out_values, cap, out_err, &dp, &pk, &gp};
    return route_batch64(ix, rq, to, out_dest_offsets);
}

// 32-bit offsets (include/tmatch.h).  An in-place batch the one-launch small
// kernel takes runs on 32-bit offsets end to end (k_walk_small<.., uint32_t>):
// half the offset bytes cross PCIe in each direction.  Any other batch is
// widened on the host, matched as tm_match_batch_ex, and narrowed.
int tm_match_batch32_ex(tm_index *ix, uint64_t n, const uint8_t *tb, const uint32_t *to, uint32_t *out_hit,
                        uint32_t *out_vals, uint64_t cap, uint8_t *out_err, uint32_t order, uint32_t *out_unique) {
    if (!ix) return fail(nullptr, TM_EINVAL, "tm_match_batch32: null handle");
    if (!to || !out_hit || (n && !tb && to[n] != to[0])) return fail(ix, TM_EINVAL, "tm_match_batch32: null buffer");
    if (n >= 0xFFFFFFFFull) return fail(ix, TM_EINVAL, "tm_match_batch32: batch too large");
    if (order > TM_ORDER_UNIQUE) return fail(ix, TM_EINVAL, "tm_match_batch32: bad order");
    if (cap > 0xFFFFFFFFull) cap = 0xFFFFFFFFull;   // (a 32-bit offset addresses no more)
    if (n && n <= ZC_TOPICS && order == TM_ORDER_TRAVERSAL && ((uintptr_t)tb & 15) == 0) {
        const uint64_t nbytes = to[n];   // (before the lock: in TM_ALLOC_VRAM memory a host read is a PCIe round trip)
        HostBatch hb(ix);
        bool ok = tb || !nbytes;
        uint8_t *db = opt_dev(ix, tb, nbytes, ok);
        uint8_t *dof = opt_dev(ix, to, (n + 1) * 4, ok);
        uint8_t *dh = opt_dev(ix, out_hit, (n + 1) * 4, ok);
        uint8_t *dv = opt_dev(ix, out_vals, cap * 4, ok);
        uint8_t *de = opt_dev(ix, out_err, n, ok);
        if (ok) {
            if (ix->cmb_leaders > 0 && de) {   // through the combiner (the flags have a home)
                hb.g.unlock();
                SmallReq rq;
                rq.n = n; rq.db = db; rq.dof = dof; rq.dh = dh; rq.de = de; rq.dv = dv; rq.cap = dv ? cap : 0;
                const int rc = small_combined(ix, rq);
                if (rc != CMB_LEGACY) {
                    if (rc) return rc;
                    return (out_vals && out_hit[n] > cap) ? TM_ECAP : TM_OK;
                }
                hb.g.lock();
            }
            int rc;
            if ((rc = hb.open(n))) return rc;
            Lane &ln = *hb.ln;
            if (small_path_ok(dev_view(ix, ln.r), n)) {
                ix->rep[ln.r].batches++;
                if (!de && (rc = stage_out(ix, ln, n, n, de))) return rc;   // flags nobody reads still need a home
                rc = hb.run([&](const DevIndex &d, uint32_t tag) -> int {
                    int path = PATH_SMALL;
                    HIPCHK(ix, launch_match32(d, ln.w, n, db ? db : dof, reinterpret_cast<const uint32_t *>(dof),
                                              reinterpret_cast<uint32_t *>(dh), de, reinterpret_cast<uint32_t *>(dv),
                                              dv ? cap : 0, tag, next_lb(ix), ix->small_kind, ln.s, &path));
                    ix->path_batches[path]++;
                    return TM_OK;
                });
                if (rc) return rc;
                return (out_vals && out_hit[n] > cap) ? TM_ECAP : TM_OK;
            }
        }
    }
    // widened: the 64-bit path, then the offsets narrowed.  Offsets in
    // TM_ALLOC_VRAM memory are widened on the device (the host never reads
    // them: ADVICE r5 -- a deep index, > 65536 topics or a sorted order took
    // this path and read the NIF's device buffers back over the BAR)
    bool voffs;
    {
        std::lock_guard<std::mutex> g(ix->mu);
        voffs = vram_buf(ix, to, (n + 1) * 4) != nullptr;
    }
    std::vector<uint64_t> o64, h64;
    try {
        if (!voffs) o64.assign(to, to + n + 1);
        h64.resize(n + 1);
    } catch (const std::bad_alloc &) {
        return fail(ix, TM_ENOMEM, "tm_match_batch32: out of host memory");
    }
    const int rc = voffs ? match_batch_impl(ix, n, tb, nullptr, to, h64.data(), out_vals, cap, out_err, order, out_unique)
                         : tm_match_batch_ex(ix, n, tb, o64.data(), h64.data(), out_vals, cap, out_err, order, out_unique);
    if (rc != TM_OK && rc != TM_ECAP) return rc;
    if (h64[n] > 0xFFFFFFFFull) return fail(ix, TM_EINVAL, "tm_match_batch32: more than 2^32 - 1 values");
    for (uint64_t i = 0; i <= n; i++) out_hit[i] = (uint32_t)h64[i];
    return rc;
}

// (offset, count) pairs (include/tmatch.h): an in-place batch the one-launch
// kernel takes runs through the combiner as a pairs launch -- no look-back,
// so no block waits for another; any other batch takes the CSR path and is
// converted on the host.
int tm_match_batch32_pairs(tm_index *ix, uint64_t n, const uint8_t *tb, const uint32_t *to, uint32_t *out_pairs,
                           uint32_t *out_vals, uint64_t cap, uint8_t *out_err) {
    if (!ix) return fail(nullptr, TM_EINVAL, "tm_match_batch32_pairs: null handle");
    if (!to || !out_pairs || !out_err || (n && !tb && to[n] != to[0]))
        return fail(ix, TM_EINVAL, "tm_match_batch32_pairs: null buffer");
    if (n >= 0x7FFFFFFFull) return fail(ix, TM_EINVAL, "tm_match_batch32_pairs: batch too large");
    if (cap > 0xFFFFFFFFull) cap = 0xFFFFFFFFull;
    if (!n) { out_pairs[0] = 0; return TM_OK; }
    if (n <= ZC_TOPICS && ((uintptr_t)tb & 15) == 0) {
        const uint64_t nbytes = to[n];   // (before the lock: in TM_ALLOC_VRAM memory a host read is a PCIe round trip)
        SmallReq rq;
        bool ok = tb || !nbytes;
        {
            std::lock_guard<std::mutex> g(ix->mu);
            rq.db = opt_dev(ix, tb, nbytes, ok);
            rq.dof = opt_dev(ix, to, (n + 1) * 4, ok);
            rq.dh = opt_dev(ix, out_pairs, (2 * n + 1) * 4, ok);
            rq.dv = opt_dev(ix, out_vals, cap * 4, ok);
            rq.de = opt_dev(ix, out_err, n, ok);
        }
        if (ok) {
            rq.n = n; rq.cap = rq.dv ? cap : 0; rq.pairs = true;
            uint64_t t_end = 0;   // (TM_DEBUG_COMBINE 0: every batch its own launch)
            const int rc = ix->cmb_leaders.load() > 0 ? small_combined(ix, rq)
                                                      : run_small_group(ix, std::vector<SmallReq *>{&rq}, &t_end);
            if (rc != CMB_LEGACY) {
                if (rc) return rc;
                return (out_vals && out_pairs[2 * n] > cap) ? TM_ECAP : TM_OK;
            }
        }
    }
    std::vector<uint32_t> h;
    try {
        h.resize(n + 1);
    } catch (const std::bad_alloc &) {
        return fail(ix, TM_ENOMEM, "tm_match_batch32_pairs: out of host memory");
    }
    const int rc = tm_match_batch32_ex(ix, n, tb, to, h.data(), out_vals, cap, out_err, TM_ORDER_TRAVERSAL, nullptr);
    if (rc != TM_OK && rc != TM_ECAP) return rc;
    for (uint64_t i = 0; i < n; i++) { out_pairs[2 * i] = h[i]; out_pairs[2 * i + 1] = h[i + 1] - h[i]; }
    out_pairs[2 * n] = h[n];
    return rc;
}

// ---- the route family in place (include/tmatch.h): a 32-bit micro-batch whose
// buffers all lie in tm_host_alloc memory is matched as ONE pairs segment of
// the one-launch kernel (launch_small_segs, no combiner) into the lane's HBM
// scratch, and one-workgroup kernels write the caller's mapped outputs -- one
// synchronisation, no copy; the device never reads a caller's output.
// ROUTE32_OTHER: the batch is not eligible (the caller takes route_batch_impl).
constexpr int ROUTE32_OTHER = 1;   // (not a TM_ code)
constexpr int DP1_GRID_HEAD = DP1_ST_WORDS;   // status word of the [M, T] a grid dispatch leaves (8-byte aligned)
constexpr int SH1_HOST = DP1_GRID_HEAD + 4;   // k_sh_one's status words (its head 8-byte aligned)
constexpr int GS1_HOST = SH1_HOST + SH1_ST_WORDS;        // k_gs_one's status words
constexpr int GS1_GRID_HEAD = GS1_HOST + GS1_ST_WORDS;   // the [M, T, G, W] a grid dispatch and grouping leave
constexpr int PD1_HOST = GS1_GRID_HEAD + 8;              // k_pd_gate's status words
constexpr int GP1_HOST = PD1_HOST + PD1_ST_WORDS;        // k_gp_one's status words
constexpr int DP1_HOST_WORDS = GP1_HOST + GP1_ST_WORDS;
// the lane's device words (Lane::fo1_s): the two status pairs, then k_dp_one's head under a grouping
// request and the grid grouping's [G, W] behind it
constexpr int FO1S_HEAD = 2 * FO1_ST_WORDS;
constexpr int FO1S_GATE = FO1S_HEAD + 8;   // k_pd_gate's word: 0 go, else skip (k_sh_one's fail word, k_gp_one's gate)
constexpr int FO1S_WORDS = FO1S_GATE + 2;
static_assert(DP1_GRID_HEAD % 2 == 0, "the grid dispatch's head is two u64");
static_assert((SH1_HOST + SH1_ST_HEAD) % 2 == 0, "the pick's head is two u64");
static_assert(GS1_GRID_HEAD % 2 == 0 && FO1S_HEAD % 2 == 0, "the grouping's heads are u64");

// The device addresses of one request's buffers.  An absent or empty optional
// buffer is null (opt_dev); the delivery arrays, the head, out_member and the
// key arrays are looked at only when the request has a dispatch / a pick.
struct Route32Dev {
    const uint8_t *bytes, *offs;
    uint32_t *fo, *topic, *value;
    uint8_t *err;
    uint64_t dcap;
    uint64_t *head;
    uint32_t *dtopic, *dvalue, *dsub;
    uint32_t *member;
    const uint32_t *kc, *kt;
    uint64_t *ghead;
    uint32_t *gsub, *goff;
};

// fills `v` (caller holds ix->mu: the list of tm_host_alloc buffers);
// false: a buffer lies elsewhere, the batch is staged
static bool route32_resolve(tm_index *ix, const RouteReq &rq, const uint32_t *to, uint64_t nbytes,
                            uint32_t *out_dest_offsets, Route32Dev &v) {
    const RouteDispatch *dp = rq.dp;
    const RoutePick *pk = rq.pk;
    const RouteGroup *gp = rq.gp;
    bool ok = rq.tb || !nbytes;
    const auto words = [&](const void *p, uint64_t k) { return reinterpret_cast<uint32_t *>(opt_dev(ix, p, k * 4, ok)); };
    v.bytes = opt_dev(ix, rq.tb, nbytes, ok);
    v.offs = opt_dev(ix, to, (rq.n + 1) * 4, ok);
    v.fo = words(out_dest_offsets, (uint64_t)rq.n_dests + 2);
    v.topic = words(rq.out_topic, rq.cap);
    v.value = words(rq.out_values, rq.cap);
    v.err = pinned_dev(ix, rq.out_err, rq.n);   // (required even for no topics)
    v.dcap = dp ? std::min<uint64_t>(dp->dcap, 0xFFFFFFFFull) : 0;
    v.head = dp ? reinterpret_cast<uint64_t *>(pinned_dev(ix, dp->out_head, 16)) : nullptr;
    v.dtopic = dp ? words(dp->out_topic, v.dcap) : nullptr;
    v.dvalue = dp ? words(dp->out_value, v.dcap) : nullptr;
    v.dsub = dp ? words(dp->out_sub, v.dcap) : nullptr;
    v.member = pk ? words(pk->out_member, rq.cap) : nullptr;
    v.kc = pk ? words(pk->key_clientid, rq.n) : nullptr;
    v.kt = pk ? words(pk->key_topic, rq.n) : nullptr;
    v.ghead = gp ? reinterpret_cast<uint64_t *>(pinned_dev(ix, gp->out_ghead, 16)) : nullptr;
    v.gsub = gp ? words(gp->out_gsub, gp->gcap) : nullptr;
    v.goff = gp ? reinterpret_cast<uint32_t *>(pinned_dev(ix, gp->out_goff32, (gp->gcap + 1) * 4)) : nullptr;
    return ok && v.err && (!dp || v.head) && (!gp || (v.ghead && v.goff));
}

// room on the lane for one attempt with vcap values: the match's pairs and
// values; under aggre or dp k_fo_one's results, which then stay on the device
// (k_ag_one / k_dp_one writes the caller's buffers); under both k_ag_one's too
static int route32_scratch(tm_index *ix, Lane &ln, const RouteReq &rq, uint64_t vcap) {
    int rc;
    const hipStream_t s = ln.s;
    const uint64_t nfo = (uint64_t)rq.n_dests + 2;
    if ((rc = grow_dev(ix, s, ln.d_vals, ln.d_vals_cap, vcap))) return rc;
    if ((rc = grow_dev(ix, s, ln.d_pr, ln.d_pr_cap, 2 * rq.n + 2))) return rc;
    if (rq.aggre() || rq.dp) {
        if ((rc = grow_dev(ix, s, ln.d_ft, ln.d_ft_cap, FO1_ENTRIES))) return rc;
        if ((rc = grow_dev(ix, s, ln.d_fv, ln.d_fv_cap, FO1_ENTRIES))) return rc;
        if ((rc = grow_dev(ix, s, ln.d_fo, ln.d_fo_cap, nfo))) return rc;
    }
    if (rq.aggre() && rq.dp) {
        if ((rc = grow_dev(ix, s, ln.d_at, ln.d_at_cap, FO1_ENTRIES))) return rc;
        if ((rc = grow_dev(ix, s, ln.d_av, ln.d_av_cap, FO1_ENTRIES))) return rc;
        if ((rc = grow_dev(ix, s, ln.d_ao, ln.d_ao_cap, nfo))) return rc;
    }
    if (rq.gp) {   // k_dp_one's deliveries stay on the lane: k_gs_one writes the caller's
        if ((rc = grow_dev(ix, s, ln.d_dt, ln.d_dt_cap, GS1_DELIVERIES))) return rc;
        if ((rc = grow_dev(ix, s, ln.d_dv, ln.d_dv_cap, GS1_DELIVERIES))) return rc;
        if ((rc = grow_dev(ix, s, ln.d_ds, ln.d_ds_cap, GS1_DELIVERIES))) return rc;
    }
    // k_sh_one's picks stay on the lane too: k_gp_one copies them out and merges them
    if (rq.gp && rq.pk && (rc = grow_dev(ix, s, ln.d_sm, ln.d_sm_cap, FO1_ENTRIES))) return rc;
    return TM_OK;
}

// Queues one attempt on the lane's stream (caller holds ix->mu): the segment
// walk, the flags into the caller's out_err, then k_fo_one.  A plain route:
// k_fo_one fans out into the caller's outputs -- two launches.  aggre alone:
// k_fo_one's results stay on the lane and k_ag_one writes the outputs.  dp:
// k_ag_one's (if any) stay there too, and ONE more launch of one workgroup,
// k_dp_one, writes the route outputs, the head and the deliveries.  pk: in the
// same lock hold, on the same stream, the share tables of this very run's
// snapshot and ONE more workgroup, k_sh_one, over k_ag_one's entries.  The run
// may be run again (a value scratch that grows, a look-back retry), so
// k_sh_one gates itself on the device (tm_dev.h launch_share_one) and reports
// into the lane's status block.  gp: k_dp_one is the same code with other
// pointers -- its deliveries and its head go to the lane, it expands up to
// min(dp1_max, gs1_max) deliveries -- and ONE more workgroup, k_gs_one, groups
// them into the caller's buffers (tm_dev.h launch_group_one); it moves no
// state, so a run queued again just writes again.  pk and gp
// (tm_publish_deliver_batch32): k_dp_one as under gp, then k_pd_gate, which
// decides once on the device whether the run stands and fits, k_sh_one with
// the gate's word for its fail word and the lane's d_sm for its out_member,
// and k_gp_one, which copies the picks out, merges the local ones with the
// deliveries and groups them into the caller's buffers (tm_dev.h
// launch_group_picks_one) -- the pick is made exactly when the merge runs.
static int route32_queue(tm_index *ix, Lane &ln, const RouteReq &rq, const Route32Dev &v, const DevIndex &d,
                         uint32_t tag, uint64_t vcap) {
    int rc;
    const hipStream_t s = ln.s;
    const uint64_t n = rq.n, cap = rq.cap;
    const uint32_t n_dests = rq.n_dests;
    const bool aggre = rq.aggre();
    const RouteDispatch *dp = rq.dp;
    volatile uint32_t *st = ln.fo1_h;
    if (n) {
        SmallSegs sg{};
        sg.count = 1;
        sg.pairs = 1;
        sg.s[0] = SmallSeg{v.bytes ? v.bytes : v.offs, v.offs, ln.d_pr, v.err, ln.d_vals, vcap, (uint32_t)n, 0};
        int path = PATH_SMALL;
        HIPCHK(ix, launch_small_segs(d, ln.w, sg, true, tag, next_lb(ix), ix->small_kind, s, &path));
        ix->path_batches[path]++;
    }
    const int grp = ix->rep[ln.r].group;
    const uint32_t *dtab = nullptr, *ftab = nullptr;
    uint64_t dlen = 0, flen = 0;
    if ((rc = dest_upload(ix, grp, s, dtab, dlen))) return rc;
    st[FO1_ST_STATE] = 0;   // (the lane's stream is idle: nothing else writes the words)
    st[SH1_HOST + SH1_ST_STATE] = 0;
    st[GS1_HOST + GS1_ST_STATE] = 0;
    st[PD1_HOST + PD1_ST_STATE] = 0;
    st[GP1_HOST + GP1_ST_STATE] = 0;
    if (!aggre && !dp) {
        HIPCHK(ix, launch_fanout_one(n, ln.d_pr, ln.d_vals, vcap, dtab, dlen, n_dests, v.fo, v.topic, v.value, cap,
                                     ln.fo1_d, s));
        return TM_OK;
    }
    if (aggre && (rc = filter_upload(ix, grp, s, ftab, flen))) return rc;
    uint32_t *lfo = reinterpret_cast<uint32_t *>(ln.d_fo);
    HIPCHK(ix, launch_fanout_one(n, ln.d_pr, ln.d_vals, vcap, dtab, dlen, n_dests, lfo, ln.d_ft, ln.d_fv, FO1_ENTRIES,
                                 ln.fo1_s, s));
    if (!dp) {
        HIPCHK(ix, launch_aggre_one(ln.fo1_s, lfo, n_dests, ln.d_ft, ln.d_fv, ftab, flen, v.fo, v.topic, v.value, cap,
                                    ln.fo1_d, s));
        return TM_OK;
    }
    uint32_t *lao = nullptr, *st_dev = ln.fo1_s;
    if (aggre) {   // (room for every entry k_fo_one completes: the pass always compacts)
        lao = reinterpret_cast<uint32_t *>(ln.d_ao);
        st_dev = ln.fo1_s + FO1_ST_WORDS;
        HIPCHK(ix, launch_aggre_one(ln.fo1_s, lfo, n_dests, ln.d_ft, ln.d_fv, ftab, flen, lao, ln.d_at, ln.d_av,
                                    FO1_ENTRIES, st_dev, s));
    }
    const uint32_t *span = nullptr, *pool = nullptr;
    uint64_t span_len = 0, pool_len = 0;
    if ((rc = subs_upload(ix, grp, s, span, span_len, pool, pool_len))) return rc;
    if (const RouteGroup *gp = rq.gp) {
        uint64_t *lhead = reinterpret_cast<uint64_t *>(ln.fo1_s + FO1S_HEAD);
        const uint64_t ldcap = std::min<uint64_t>(v.dcap, GS1_DELIVERIES);
        const uint64_t lmax = std::min({ix->dp1_max, ix->gs1_max, rq.pk ? ix->gp1_max : ix->gs1_max});
        HIPCHK(ix, launch_dispatch_one(st_dev, lfo, ln.d_ft, ln.d_fv, lao, ln.d_at, ln.d_av, n_dests, dp->local_dest, span,
                                       span_len, pool, pool_len, v.fo, v.topic, v.value, cap, lhead, ln.d_dt, ln.d_dv,
                                       ln.d_ds, ldcap, lmax, ln.fo1_d, s));
        if (const RoutePick *pk = rq.pk) {
            // tm_publish_deliver_batch32 (pk requires aggre: lao is k_ag_one's).  The share tables and the
            // member-subs table of this very run's snapshot; the gate decides once for the pick and the merge
            const uint32_t *slot_of = nullptr, *rec = nullptr, *spool = nullptr, *sub_of = nullptr;
            uint64_t slot_len = 0, n_slots = 0, spool_len = 0, sub_of_len = 0;
            uint32_t *state = nullptr, *gate = ln.fo1_s + FO1S_GATE;
            if ((rc = share_upload(ix, grp, s, slot_of, slot_len, rec, n_slots, spool, spool_len, state))) return rc;
            if ((rc = msub_upload(ix, grp, s, sub_of, sub_of_len))) return rc;
            HIPCHK(ix, launch_pd_gate(st_dev, lhead, lao, n_dests, n ? ln.w.hint_d + HINT_FAIL : nullptr, vcap, cap, v.dcap,
                                      lmax, ix->gp1_max, v.head, gate, ln.fo1_d + PD1_HOST, s));
            HIPCHK(ix, launch_share_one(st_dev, gate, lao, n_dests, ln.d_at, ln.d_av, vcap, cap, v.kc, v.kt, n, pk->seed,
                                        slot_of, slot_len, rec, n_slots, spool, spool_len, state, ln.d_sm,
                                        ln.fo1_d + SH1_HOST, s));
            HIPCHK(ix, launch_group_picks_one(gate, lhead, ln.d_dt, ln.d_dv, ln.d_ds, lao, n_dests, ln.d_at, ln.d_av,
                                              ln.d_sm, sub_of, sub_of_len, cap, v.dcap, v.member, v.dtopic, v.dvalue,
                                              v.dsub, v.ghead, v.gsub, v.goff, gp->gcap, ln.fo1_d + GP1_HOST, s));
            return TM_OK;
        }
        HIPCHK(ix, launch_group_one(st_dev, lhead, ln.d_dt, ln.d_dv, ln.d_ds, ldcap, lmax, v.head, v.dtopic, v.dvalue,
                                    v.dsub, v.ghead, v.gsub, v.goff, gp->gcap, ln.fo1_d + GS1_HOST, s));
        return TM_OK;
    }
    HIPCHK(ix, launch_dispatch_one(st_dev, lfo, ln.d_ft, ln.d_fv, lao, ln.d_at, ln.d_av, n_dests, dp->local_dest, span,
                                   span_len, pool, pool_len, v.fo, v.topic, v.value, cap, v.head, v.dtopic, v.dvalue,
                                   v.dsub, v.dcap, ix->dp1_max, ln.fo1_d, s));
    if (!rq.pk) return TM_OK;
    const uint32_t *slot_of = nullptr, *rec = nullptr, *spool = nullptr;
    uint64_t slot_len = 0, n_slots = 0, spool_len = 0;
    uint32_t *state = nullptr;
    if ((rc = share_upload(ix, grp, s, slot_of, slot_len, rec, n_slots, spool, spool_len, state))) return rc;
    HIPCHK(ix, launch_share_one(st_dev, n ? ln.w.hint_d + HINT_FAIL : nullptr, lao, n_dests, ln.d_at, ln.d_av, vcap, cap,
                                v.kc, v.kt, n, rq.pk->seed, slot_of, slot_len, rec, n_slots, spool, spool_len, state,
                                v.member, ln.fo1_d + SH1_HOST, s));
    return TM_OK;
}

// k_sh_one's status against the host's view of the run that stands: it picked
// (and moved the state, once) exactly when the caller gets the entries --
// total <= cap and the fan-out completed
static int route32_pick_status(tm_index *ix, Lane &ln, const RouteReq &rq, uint64_t total, uint32_t state) {
    const uint32_t ps = ln.fo1_h[SH1_HOST + SH1_ST_STATE];
    const bool want = total <= rq.cap && (state == FO1_DONE || state == (uint32_t)DP1_TOO_LARGE);
    if ((ps != SH1_PICKED && ps != SH1_SKIPPED) || (ps == SH1_PICKED) != want)
        return route_fail(ix, rq, TM_EDEVICE, "the pick kernel and the host disagree on whether the run stands");
    if (want) ix->publish_one++;
    return TM_OK;
}

// k_gs_one's status against the host's view of the run that stands: it grouped
// exactly when k_dp_one expanded the deliveries (FO1_DONE)
static int route32_group_status(tm_index *ix, Lane &ln, const RouteReq &rq, uint32_t state) {
    const uint32_t gs = ln.fo1_h[GS1_HOST + GS1_ST_STATE];
    if ((gs != GS1_GROUPED && gs != GS1_SKIPPED) || (gs == GS1_GROUPED) != (state == FO1_DONE))
        return route_fail(ix, rq, TM_EDEVICE, "the grouping kernel and the host disagree on whether the dispatch expanded");
    return TM_OK;
}

// ending 1, FO1_DONE: everything is in the caller's buffers
static int route32_end_in_place(tm_index *ix, Lane &ln, const RouteReq &rq, uint64_t total) {
    if (!rq.dp) {
        ix->route_one++;
        return total > rq.cap ? TM_ECAP : TM_OK;
    }
    const volatile uint32_t *st = ln.fo1_h;
    const uint64_t T = (uint64_t)st[DP1_ST_T_HI] << 32 | st[DP1_ST_T_LO];
    if (rq.gp) {
        ix->deliver_one++;
        ix->gs1_passes[0] += st[GS1_HOST + GS1_ST_RUN];
        ix->gs1_passes[1] += st[GS1_HOST + GS1_ST_SKIPPED];
        return total > rq.cap || T > rq.dp->dcap || st[GS1_HOST + GS1_ST_G] > rq.gp->gcap ? TM_ECAP : TM_OK;
    }
    ix->dispatch_one++;
    return total > rq.cap || T > rq.dp->dcap ? TM_ECAP : TM_OK;
}

// A grid ending under a grouping request (caller holds the lock, which is
// dropped for the wait; `doff`: the final bucket offsets on the lane, whatever
// comes before them already queued): the grid dispatch of the local bucket
// into the lane's delivery scratch and the grid grouping behind it, as
// route_batch_impl queues them; head = [M, T, G, W].  dwant: the deliveries the
// lane makes room for at first -- T where k_dp_one left it; more than that and
// the two run again on the arrays still on the lane.
static int route32_grid_group(tm_index *ix, HostBatch &hb, const RouteReq &rq, const uint64_t *doff, bool aggre,
                              uint64_t vcap, uint64_t dwant, uint64_t head[4]) {
    int rc;
    Lane &ln = *hb.ln;
    const hipStream_t s = ln.s;
    const RouteDispatch *dp = rq.dp;
    const uint64_t dcap = std::min<uint64_t>(dp->dcap, 0xFFFFFFFFull), gcap = rq.gp->gcap;
    uint64_t *lhead = reinterpret_cast<uint64_t *>(ln.fo1_s + FO1S_HEAD);
    dwant = std::min(dwant, dcap);
    for (int attempt = 0;; attempt++) {
        if ((rc = dispatch_scratch(ix, ln, vcap, dwant))) return rc;
        if ((rc = group_scratch(ix, ln, dwant, gcap, rq.who))) return rc;
        if ((rc = queue_dispatch_to(ix, ln, rq.n_dests, dp->local_dest, doff, aggre, vcap, dwant, lhead, ln.d_dt, ln.d_dv,
                                    ln.d_ds)))
            return rc;
        if ((rc = queue_group(ix, ln, lhead, dwant, gcap, lhead + 2))) return rc;
        HIPCHK(ix, hipMemcpyAsync(ln.fo1_h + GS1_GRID_HEAD, lhead, 32, hipMemcpyDeviceToHost, s));
        if ((rc = batch_done(ix, ln))) return rc;
        hb.g.unlock();
        HIPCHK(ix, hipStreamSynchronize(s));
        std::memcpy(head, ln.fo1_h + GS1_GRID_HEAD, 32);
        if (std::min(head[1], dcap) <= dwant) return TM_OK;
        if (attempt >= 2) return route_fail(ix, rq, TM_EDEVICE, "the delivery total kept growing past the scratch");
        dwant = std::min(head[1] + head[1] / 4, dcap);
        if ((rc = hb.relock())) return rc;
    }
}

// what route32_grid_group left on the lane, to the caller (the lock is not held)
static int route32_group_out(tm_index *ix, Lane &ln, const RouteReq &rq, const uint64_t head[4], uint64_t total) {
    if (int rc = copy_group_out(ix, ln, rq, head)) return rc;
    ix->deliver_grid++;
    return total > rq.cap || head[1] > rq.dp->dcap || head[2] > rq.gp->gcap ? TM_ECAP : TM_OK;
}

// the [M, T] a grid dispatch left with the lane's status words, to the caller
static int route32_grid_head(tm_index *ix, Lane &ln, const RouteReq &rq, uint64_t total) {
    const volatile uint64_t *gh = reinterpret_cast<const volatile uint64_t *>(ln.fo1_h + DP1_GRID_HEAD);
    rq.dp->out_head[0] = gh[0];
    rq.dp->out_head[1] = gh[1];
    ix->dispatch_grid++;
    return total > rq.cap || gh[1] > rq.dp->dcap ? TM_ECAP : TM_OK;
}

// ending 2, DP1_TOO_LARGE: more deliveries than one workgroup should write
// (dp1_max).  The route outputs are in place (and under pk the picks are
// made); the grid kernels (launch_dispatch) expand the bucket of the arrays on
// the lane (their u32 offsets widened beside them) straight into the caller's
// buffers
static int route32_end_grid_dispatch(tm_index *ix, HostBatch &hb, const RouteReq &rq, const Route32Dev &v, uint64_t total) {
    int rc;
    Lane &ln = *hb.ln;
    const hipStream_t s = ln.s;
    const bool aggre = rq.aggre();
    const uint64_t nfo = (uint64_t)rq.n_dests + 2;
    if ((rc = hb.relock())) return rc;
    if ((rc = ensure_dispatch(ix, ln, FO1_ENTRIES, true))) return rc;
    if ((rc = grow_dev(ix, s, ln.d_o64, ln.d_o64_cap, nfo))) return rc;
    HIPCHK(ix, launch_offs_widen(reinterpret_cast<const uint32_t *>(aggre ? ln.d_ao : ln.d_fo), ln.d_o64, nfo, s));
    if (rq.gp) {   // into the lane's scratch, grouped there, copied out
        const volatile uint32_t *st = ln.fo1_h;
        const uint64_t T = (uint64_t)st[DP1_ST_T_HI] << 32 | st[DP1_ST_T_LO];
        uint64_t head[4];
        if ((rc = route32_grid_group(ix, hb, rq, ln.d_o64, aggre, FO1_ENTRIES, T, head))) return rc;
        return route32_group_out(ix, ln, rq, head, total);
    }
    if ((rc = queue_dispatch_to(ix, ln, rq.n_dests, rq.dp->local_dest, ln.d_o64, aggre, FO1_ENTRIES, v.dcap,
                                reinterpret_cast<uint64_t *>(ln.fo1_d + DP1_GRID_HEAD), v.dtopic, v.dvalue, v.dsub)))
        return rc;
    if ((rc = batch_done(ix, ln))) return rc;
    hb.g.unlock();
    HIPCHK(ix, hipStreamSynchronize(s));
    return route32_grid_head(ix, ln, rq, total);
}

// ending 3, FO1_TOO_LARGE: more entries than k_fo_one takes.  The grid kernels
// run on the same pairs (no second walk) into the lane's scratch, copied out
// and narrowed; a dispatch writes the deliveries straight into the caller's
// buffers; a pick follows as in route_batch_impl (pick_after_run).
// (under aggre with total > cap: TM_ECAP, the un-aggregated sizes, no entries;
// a dispatch reads the aggregated arrays all the same)
static int route32_end_grid(tm_index *ix, HostBatch &hb, const RouteReq &rq, const Route32Dev &v,
                            uint32_t *out_dest_offsets, uint64_t total, uint64_t vcap) {
    int rc;
    Lane &ln = *hb.ln;
    const uint32_t n_dests = rq.n_dests;
    const RouteDispatch *dp = rq.dp;
    const bool ag_out = rq.aggre() && total <= rq.cap, ag = rq.aggre() && (dp || ag_out);
    std::vector<uint64_t> fo;
    try {
        fo.resize((uint64_t)n_dests + 2);
    } catch (const std::bad_alloc &) {
        return route_fail(ix, rq, TM_ENOMEM, "out of host memory");
    }
    if ((rc = hb.relock())) return rc;
    if ((rc = route_scratch(ix, ln, n_dests, vcap, ag, true, rq.n))) return rc;
    if (dp && (rc = ensure_dispatch(ix, ln, vcap, true))) return rc;
    if ((rc = queue_grid_fanout(ix, ln, rq.n, nullptr, ln.d_pr, vcap, n_dests, ag))) return rc;
    uint64_t ghead[4] = {0, 0, 0, 0};
    if (rq.gp) {
        if ((rc = route32_grid_group(ix, hb, rq, ag ? ln.d_ao : ln.d_fo, ag, vcap, std::max<uint64_t>(ln.d_ds_cap, 1 << 16),
                                     ghead)))
            return rc;
    } else {
        if (dp && (rc = queue_dispatch_to(ix, ln, n_dests, dp->local_dest, ag ? ln.d_ao : ln.d_fo, ag, vcap, v.dcap,
                                          reinterpret_cast<uint64_t *>(ln.fo1_d + DP1_GRID_HEAD), v.dtopic, v.dvalue,
                                          v.dsub)))
            return rc;
        if ((rc = batch_done(ix, ln))) return rc;
        hb.g.unlock();
    }
    rc = copy_route_out(ix, ln, n_dests, total, rq.cap, rq.aggre(), ag_out, fo.data(), out_dest_offsets, rq.out_topic,
                        rq.out_values);
    if (rc != TM_OK && rc != TM_ECAP) return rc;
    if (rq.pk && ag_out)
        if (int prc = pick_after_run(ix, hb, rq, vcap, std::min(fo[n_dests + 1], rq.cap))) return prc;
    if (rq.pk) ix->publish_grid++;
    if (rq.gp) return route32_group_out(ix, ln, rq, ghead, total);
    if (dp) return route32_grid_head(ix, ln, rq, total);
    ix->route_grid++;
    return rc;
}

// tm_publish_deliver_batch32's grid endings, their common tail (the lock is
// held when gm.locked; the lane holds the deliveries and d_head = [M, T]): the
// pick, the merge and the grouping exactly once (pick_after_run), then the
// grouped arrays copied out and narrowed
static int route32_pd_tail(tm_index *ix, HostBatch &hb, const RouteReq &rq, uint64_t vcap, uint64_t kept, PickMerge gm) {
    Lane &ln = *hb.ln;
    gm.pin = reinterpret_cast<uint8_t *>(ln.fo1_h + GS1_GRID_HEAD);
    gm.fetch = true;
    if (int rc = pick_after_run(ix, hb, rq, vcap, kept, &gm)) return rc;
    uint64_t head[4];
    std::memcpy(head, ln.fo1_h + GS1_GRID_HEAD, 32);
    if (int rc = copy_group_out(ix, ln, rq, head)) return rc;
    ix->publish_deliver_grid++;
    return head[2] > rq.gp->gcap ? TM_ECAP : TM_OK;
}

// The endings of tm_publish_deliver_batch32 in place.  The host's own view of
// the run that stands (the loop is over: total <= vcap, no look-back failure)
// against the three kernels' status words: the gate said go, k_sh_one picked
// and k_gp_one grouped exactly when the run hands over its entries (total <=
// cap), T + K fits dcap and one workgroup takes them.
//   one workgroup   everything is in the caller's buffers; or a capacity is
//                   short (total > cap, T + K > dcap): TM_ECAP, nothing moved.
//   the lane's grid T or T + K past one workgroup's limit: the aggre pass's u32
//                   offsets are widened beside the arrays, the grid dispatch
//                   runs into the lane where k_dp_one did not expand, then
//                   route32_pd_tail.
//   the pairs' grid FO1_TOO_LARGE: the grid fan-out, aggre and dispatch on the
//                   same pairs (no second walk) as route32_end_grid, the route
//                   outputs copied out and narrowed, tm_publish_deliver_batch's
//                   capacity rules, then route32_pd_tail.
static int route32_end_publish_deliver(tm_index *ix, HostBatch &hb, const RouteReq &rq, uint32_t *out_dest_offsets,
                                       uint64_t total, uint64_t vcap, uint32_t state) {
    int rc;
    Lane &ln = *hb.ln;
    const hipStream_t s = ln.s;
    const RouteDispatch *dp = rq.dp;
    const RouteGroup *gp = rq.gp;
    const uint32_t n_dests = rq.n_dests;
    const volatile uint32_t *st = ln.fo1_h;
    const uint64_t dcap = std::min<uint64_t>(dp->dcap, 0xFFFFFFFFull);
    uint64_t *lhead = reinterpret_cast<uint64_t *>(ln.fo1_s + FO1S_HEAD);
    if (state != FO1_DONE && state != (uint32_t)DP1_TOO_LARGE && state != FO1_TOO_LARGE)
        return route_fail(ix, rq, TM_EDEVICE, "the fan-out kernel left no status");
    const bool done = state != FO1_TOO_LARGE;   // k_fo_one and k_ag_one completed: T and K are known
    const uint64_t T = (uint64_t)st[DP1_ST_T_HI] << 32 | st[DP1_ST_T_LO], K = st[PD1_HOST + PD1_ST_K];
    const uint32_t pd = st[PD1_HOST + PD1_ST_STATE], ps = st[SH1_HOST + SH1_ST_STATE], gs = st[GP1_HOST + GP1_ST_STATE];
    const bool fits = done && total <= rq.cap && T + K <= dcap;
    const bool want = fits && state == FO1_DONE && T + K <= std::min<uint64_t>(ix->gp1_max, GP1_DELIVERIES);
    if ((pd != PD1_GO && pd != PD1_SKIP) || (ps != SH1_PICKED && ps != SH1_SKIPPED) ||
        (gs != GP1_GROUPED && gs != GP1_SKIPPED) || (pd == PD1_GO) != want || (ps == SH1_PICKED) != want ||
        (gs == GP1_GROUPED) != want)
        return route_fail(ix, rq, TM_EDEVICE, "the gate, the pick and the merge kernels and the host disagree on whether "
                                              "the run stands");
    if (want) {
        ix->publish_deliver_one++;
        ix->gs1_passes[0] += st[GP1_HOST + GP1_ST_RUN];
        ix->gs1_passes[1] += st[GP1_HOST + GP1_ST_SKIPPED];
        return st[GP1_HOST + GP1_ST_G] > gp->gcap ? TM_ECAP : TM_OK;
    }
    if (done && !fits) {   // nothing moved; out_head and the bucket offsets size the retry
        gp->out_ghead[0] = gp->out_ghead[1] = 0;
        ix->publish_deliver_one++;
        return TM_ECAP;
    }
    const uint64_t nfo = (uint64_t)n_dests + 2;
    if ((rc = hb.relock())) return rc;
    if (done) {
        if ((rc = ensure_dispatch(ix, ln, FO1_ENTRIES, true))) return rc;
        if ((rc = grow_dev(ix, s, ln.d_o64, ln.d_o64_cap, nfo))) return rc;
        HIPCHK(ix, launch_offs_widen(reinterpret_cast<const uint32_t *>(ln.d_ao), ln.d_o64, nfo, s));
        if (state == (uint32_t)DP1_TOO_LARGE) {   // (T <= dcap: the lane takes every delivery, no retry)
            if ((rc = dispatch_scratch(ix, ln, FO1_ENTRIES, T))) return rc;
            if ((rc = queue_dispatch_to(ix, ln, n_dests, dp->local_dest, ln.d_o64, true, FO1_ENTRIES, T, lhead, ln.d_dt,
                                        ln.d_dv, ln.d_ds)))
                return rc;
        }
        PickMerge gm{lhead, T, gp->gcap, nullptr, true, ln.d_o64, true};
        return route32_pd_tail(ix, hb, rq, FO1_ENTRIES, K, gm);
    }
    std::vector<uint64_t> fo;
    try {
        fo.resize(nfo);
    } catch (const std::bad_alloc &) {
        return route_fail(ix, rq, TM_ENOMEM, "out of host memory");
    }
    if ((rc = route_scratch(ix, ln, n_dests, vcap, true, true, rq.n))) return rc;
    if ((rc = queue_grid_fanout(ix, ln, rq.n, nullptr, ln.d_pr, vcap, n_dests, true))) return rc;
    uint64_t head[2] = {0, 0}, dwant = std::min(std::max<uint64_t>(ln.d_ds_cap, 1 << 16), dcap);
    for (int attempt = 0;; attempt++) {
        if ((rc = dispatch_scratch(ix, ln, vcap, dwant))) return rc;
        if ((rc = queue_dispatch_to(ix, ln, n_dests, dp->local_dest, ln.d_ao, true, vcap, dwant, lhead, ln.d_dt, ln.d_dv,
                                    ln.d_ds)))
            return rc;
        HIPCHK(ix, hipMemcpyAsync(ln.fo1_h + GS1_GRID_HEAD, lhead, 16, hipMemcpyDeviceToHost, s));
        if ((rc = batch_done(ix, ln))) return rc;
        hb.g.unlock();
        HIPCHK(ix, hipStreamSynchronize(s));
        std::memcpy(head, ln.fo1_h + GS1_GRID_HEAD, 16);
        if (std::min(head[1], dcap) <= dwant) break;
        if (attempt >= 2) return route_fail(ix, rq, TM_EDEVICE, "the delivery total kept growing past the scratch");
        dwant = std::min(head[1] + head[1] / 4, dcap);
        if ((rc = hb.relock())) return rc;
    }
    rc = copy_route_out(ix, ln, n_dests, total, rq.cap, true, total <= rq.cap, fo.data(), out_dest_offsets, rq.out_topic,
                        rq.out_values);
    if (rc != TM_OK && rc != TM_ECAP) return rc;
    const uint64_t kept = rc == TM_OK ? std::min(fo[n_dests + 1], rq.cap) : 0;
    dp->out_head[0] = head[0];
    dp->out_head[1] = head[1];
    gp->out_ghead[0] = gp->out_ghead[1] = 0;
    if (rc != TM_OK || head[1] + kept > dp->dcap || head[1] + kept > 0xFFFFFFFFull) {
        ix->publish_deliver_grid++;
        return TM_ECAP;
    }
    PickMerge gm{lhead, head[1], gp->gcap, nullptr, true};
    return route32_pd_tail(ix, hb, rq, vcap, kept, gm);
}

// the in-place attempt of route_batch32: the stages above, in order
static int route32_in_place(tm_index *ix, const RouteReq &rq, const uint32_t *to, uint64_t nbytes,
                            uint32_t *out_dest_offsets) {
    HostBatch hb(ix, rq.who);
    Route32Dev v;
    if (!route32_resolve(ix, rq, to, nbytes, out_dest_offsets, v)) return ROUTE32_OTHER;
    int rc;
    const uint64_t n = rq.n;
    if ((rc = hb.open(n + (uint64_t)SMALL_SEGS * SM_TOPICS))) return rc;
    Lane &ln = *hb.ln;
    if (n && !small_path_ok(dev_view(ix, ln.r), n)) return ROUTE32_OTHER;
    ix->rep[ln.r].batches++;
    if (!ln.fo1_h) {
        HIPCHK(ix, hipHostMalloc(&ln.fo1_h, DP1_HOST_WORDS * 4, hipHostMallocMapped));
        HIPCHK(ix, hipHostGetDevicePointer(reinterpret_cast<void **>(&ln.fo1_d), ln.fo1_h, 0));
    }
    if ((rq.aggre() || rq.dp) && !ln.fo1_s) HIPCHK(ix, hipMalloc(&ln.fo1_s, FO1S_WORDS * 4));
    volatile uint32_t *st = ln.fo1_h;
    uint64_t total = 0, vcap = std::max<uint64_t>({ln.d_vals_cap, 4 * n, 1 << 16});
    for (int attempt = 0;; attempt++) {
        if (vcap > 0xFFFFFFFFull) return route_fail(ix, rq, TM_EINVAL, "more than 2^32 - 1 hits in one batch");
        if ((rc = route32_scratch(ix, ln, rq, vcap))) return rc;
        rc = hb.run([&](const DevIndex &d, uint32_t tag) { return route32_queue(ix, ln, rq, v, d, tag, vcap); });
        if (rc) return rc;
        total = st[FO1_ST_TOTAL];
        if (total <= vcap) break;
        if (attempt >= 2) return route_fail(ix, rq, TM_EDEVICE, "hit total kept growing past the value scratch");
        vcap = total + total / 4;
        if ((rc = hb.relock())) return rc;
    }
    const uint32_t state = st[FO1_ST_STATE];
    if (rq.pk && rq.gp) return route32_end_publish_deliver(ix, hb, rq, out_dest_offsets, total, vcap, state);
    if (rq.pk && (rc = route32_pick_status(ix, ln, rq, total, state))) return rc;
    if (rq.gp && (rc = route32_group_status(ix, ln, rq, state))) return rc;
    if (state == FO1_DONE) return route32_end_in_place(ix, ln, rq, total);
    if (rq.dp && state == DP1_TOO_LARGE) return route32_end_grid_dispatch(ix, hb, rq, v, total);
    if (state != FO1_TOO_LARGE) return route_fail(ix, rq, TM_EDEVICE, "the fan-out kernel left no status");
    return route32_end_grid(ix, hb, rq, v, out_dest_offsets, total, vcap);
}

// The three 32-bit calls (include/tmatch.h): in place when the batch is a
// micro-batch whose buffers lie in tm_host_alloc memory; every other batch
// widened, run by route_batch_impl, and narrowed.
static int route_batch32(tm_index *ix, RouteReq rq, const uint32_t *to, uint32_t *out_dest_offsets) {
    if (int rc = route_check(ix, rq, to && out_dest_offsets, true)) return rc;
    const uint64_t n = rq.n;
    const uint64_t nbytes = n ? to[n] : 0;   // (before the lock: in TM_ALLOC_VRAM memory a host read is a PCIe round trip)
    if (n && !rq.tb && nbytes != to[0]) return route_fail(ix, rq, TM_EINVAL, "null buffer");
    if (rq.cap > 0xFFFFFFFFull) rq.cap = 0xFFFFFFFFull;   // (32-bit positions)
    if (n <= FO1_TOPICS && rq.n_dests <= FO1_MAX_DESTS && ((uintptr_t)rq.tb & 15) == 0) {
        const int rc = route32_in_place(ix, rq, to, nbytes, out_dest_offsets);
        if (rc != ROUTE32_OTHER) return rc;
    }
    // (the buffers kept per thread: a fresh 128 KB vector per call is an mmap and its page faults)
    static thread_local std::vector<uint64_t> o64, fo;
    try {
        o64.assign(to, to + n + 1);
        fo.resize((uint64_t)rq.n_dests + 2);
    } catch (const std::bad_alloc &) {
        return route_fail(ix, rq, TM_ENOMEM, "out of host memory");
    }
    const int rc = route_batch_impl(ix, rq, o64.data(), fo.data());
    if (rc != TM_OK && rc != TM_ECAP) return rc;
    for (size_t i = 0; i < fo.size(); i++) out_dest_offsets[i] = (uint32_t)fo[i];
    // (rq.gp: copy_group_out narrowed the groups' offsets into out_goff32)
    (rq.gp && rq.pk ? ix->publish_deliver_grid : rq.gp ? ix->deliver_grid : rq.pk ? ix->publish_grid :
     rq.dp ? ix->dispatch_grid : ix->route_grid)++;
    return rc;
}

int tm_route_batch32_ex(tm_index *ix, uint64_t n, const uint8_t *tb, const uint32_t *to, uint32_t n_dests,
                        uint32_t *out_dest_offsets, uint32_t *out_topic, uint32_t *out_values, uint64_t cap,
                        uint8_t *out_err, uint32_t flags) {
    return route_batch32(ix, {"tm_route_batch32_ex", n, tb, n_dests, flags, out_topic, out_values, cap, out_err, nullptr, nullptr},
                         to, out_dest_offsets);
}

int tm_route_batch32(tm_index *ix, uint64_t n, const uint8_t *tb, const uint32_t *to, uint32_t n_dests,
                     uint32_t *out_dest_offsets, uint32_t *out_topic, uint32_t *out_values, uint64_t cap,
                     uint8_t *out_err) {
    return route_batch32(ix, {"tm_route_batch32", n, tb, n_dests, 0, out_topic, out_values, cap, out_err, nullptr, nullptr}, to,
                         out_dest_offsets);
}

int tm_dispatch_batch32(tm_index *ix, uint64_t n, const uint8_t *tb, const uint32_t *to, uint32_t n_dests,
                        uint32_t local_dest, uint32_t flags, uint32_t *out_dest_offsets, uint32_t *out_topic,
                        uint32_t *out_values, uint64_t cap, uint64_t *out_head, uint32_t *out_dtopic,
                        uint32_t *out_dvalue, uint32_t *out_dsub, uint64_t dcap, uint8_t *out_err) {
    const RouteDispatch dp{local_dest, out_head, out_dtopic, out_dvalue, out_dsub, dcap};
    return route_batch32(ix, {"tm_dispatch_batch32", n, tb, n_dests, flags, out_topic, out_values, cap, out_err, &dp, nullptr},
                         to, out_dest_offsets);
}

int tm_publish_batch32(tm_index *ix, uint64_t n, const uint8_t *tb, const uint32_t *to, uint32_t n_dests,
                       uint32_t local_dest, uint32_t flags, uint32_t *out_dest_offsets, uint32_t *out_topic,
                       uint32_t *out_values, uint64_t cap, uint64_t *out_head, uint32_t *out_dtopic, uint32_t *out_dvalue,
                       uint32_t *out_dsub, uint64_t dcap, const uint32_t *key_clientid, const uint32_t *key_topic,
                       uint32_t seed, uint32_t *out_member, uint8_t *out_err) {
    const RouteDispatch dp{local_dest, out_head, out_dtopic, out_dvalue, out_dsub, dcap};
    const RoutePick pk{key_clientid, key_topic, seed, out_member};
    return route_batch32(ix, {"tm_publish_batch32", n, tb, n_dests, flags, out_topic, out_values, cap, out_err, &dp, &pk}, to,
                         out_dest_offsets);
}

int tm_deliver_batch32(tm_index *ix, uint64_t n, const uint8_t *tb, const uint32_t *to, uint32_t n_dests,
                       uint32_t local_dest, uint32_t flags, uint32_t *out_dest_offsets, uint32_t *out_topic,
                       uint32_t *out_values, uint64_t cap, uint64_t *out_head, uint32_t *out_dtopic, uint32_t *out_dvalue,
                       uint32_t *out_dsub, uint64_t dcap, uint64_t *out_ghead, uint32_t *out_gsub, uint32_t *out_goff,
                       uint64_t gcap, uint8_t *out_err) {
    const RouteDispatch dp{local_dest, out_head, out_dtopic, out_dvalue, out_dsub, dcap};
    // (G <= W < 2^32: a larger gcap asks for nothing more)
    const RouteGroup gp{out_ghead, out_gsub, nullptr, std::min<uint64_t>(gcap, 0xFFFFFFFFull), out_goff};
    return route_batch32(ix, {"tm_deliver_batch32", n, tb, n_dests, flags, out_topic, out_values, cap, out_err, &dp, nullptr, &gp},
                         to, out_dest_offsets);
}

int tm_publish_deliver_batch32(tm_index *ix, uint64_t n, const uint8_t *tb, const uint32_t *to, uint32_t n_dests,
                               uint32_t local_dest, uint32_t flags, uint32_t *out_dest_offsets, uint32_t *out_topic,
                               uint32_t *out_values, uint64_t cap, uint64_t *out_head, uint32_t *out_dtopic,
                               uint32_t *out_dvalue, uint32_t *out_dsub, uint64_t dcap, const uint32_t *key_clientid,
                               const uint32_t *key_topic, uint32_t seed, uint32_t *out_member, uint64_t *out_ghead,
                               uint32_t *out_gsub, uint32_t *out_goff, uint64_t gcap, uint8_t *out_err) {
    const RouteDispatch dp{local_dest, out_head, out_dtopic, out_dvalue, out_dsub, dcap};
    const RoutePick pk{key_clientid, key_topic, seed, out_member};
    const RouteGroup gp{out_ghead, out_gsub, nullptr, std::min<uint64_t>(gcap, 0xFFFFFFFFull), out_goff};
    return route_batch32(ix, {"tm_publish_deliver_batch32", n, tb, n_dests, flags, out_topic, out_values, cap, out_err, &dp, &pk,
                              &gp},
                         to, out_dest_offsets);
}

int tm_match_batch32_dev(tm_index *ix, uint64_t n, const uint8_t *bytes, const uint32_t *offs, uint32_t *hit_offs,
                         uint32_t *out, uint64_t cap, uint8_t *err, void *stream) {
    if (!ix) return fail(nullptr, TM_EINVAL, "tm_match_batch32_dev: null handle");
    if (!hit_offs || (n && (!offs || !bytes || !err))) return fail(ix, TM_EINVAL, "tm_match_batch32_dev: null buffer");
    if (n >= 0xFFFFFFFFull) return fail(ix, TM_EINVAL, "tm_match_batch32_dev: batch too large");
    if (cap > 0xFFFFFFFFull) cap = 0xFFFFFFFFull;
    DevBatch b(ix, stream);
    int rc;
    if ((rc = b.open_match(n))) return rc;
    Lane *ln = b.ln;
    const DevIndex &d = b.d;
    const hipStream_t s = b.s;
    const tm_index::ProfEv &ev = b.ev;
    uint32_t tag;
    if ((rc = next_tag(ix, *ln, s, tag))) return rc;
    if (small_path_ok(d, n)) {
        if (ev.w0) HIPCHK(ix, hipEventRecord(ev.w0, s));
        int path = PATH_SMALL;
        HIPCHK(ix, launch_match32(d, ln->w, n, bytes, offs, hit_offs, err, out, out ? cap : 0, tag, next_lb(ix),
                                  ix->small_kind, s, &path));
        if (ev.w1) HIPCHK(ix, hipEventRecord(ev.w1, s));
        ix->path_batches[path]++;
    } else {
        // widened into the lane's scratch, matched, narrowed into the caller's offsets
        if ((rc = grow_dev(ix, s, ln->d_o64, ln->d_o64_cap, n + 1))) return rc;
        if ((rc = grow_dev(ix, s, ln->d_h64, ln->d_h64_cap, n + 1))) return rc;
        HIPCHK(ix, launch_offs_widen(offs, ln->d_o64, n + 1, s));
        int path = PATH_PHASES;
        HIPCHK(ix, launch_match(d, ln->w, n, bytes, ln->d_o64, ln->d_h64, err, out, out ? cap : 0, tag, next_lb(ix),
                                ix->dbg_phases, ix->small_kind, s, ev.w0, ev.w1, &path));
        ix->path_batches[path]++;
        HIPCHK(ix, launch_offs_narrow(ln->d_h64, hit_offs, n + 1, s));
    }
    return b.done();
}

int tm_first_batch(tm_index *ix, uint64_t n, const uint8_t *tb, const uint64_t *to, uint32_t *out_value,
                   uint8_t *out_found) {
    if (!ix) return fail(nullptr, TM_EINVAL, "tm_first_batch: null handle");
    if (!to || !out_value || !out_found || (n && !tb && to[n] != to[0]))
        return fail(ix, TM_EINVAL, "tm_first_batch: null buffer");
    if (n >= 0xFFFFFFFFull) return fail(ix, TM_EINVAL, "tm_first_batch: batch too large");
    HostBatch hb(ix);
    int rc;
    if ((rc = hb.open(n))) return rc;
    Lane &ln = *hb.ln;
    const hipStream_t s = ln.s;
    ix->rep[ln.r].batches++;
    // (launch_first has no look-back: nothing to retry, so no run())
    if (n && n <= ZC_TOPICS) {   // tm_host_alloc buffers: in place
        const uint64_t nbytes = to[n];
        bool ok = tb || !nbytes;
        uint8_t *db = opt_dev(ix, tb, nbytes, ok);
        uint8_t *dof = opt_dev(ix, to, (n + 1) * 8, ok);
        uint8_t *dv = opt_dev(ix, out_value, n * 4, ok);
        uint8_t *df = opt_dev(ix, out_found, n, ok);
        const bool aligned = ((uintptr_t)tb & 15) == 0;
        if (ok && aligned) {
            HIPCHK(ix, launch_first(dev_view(ix, ln.r), ln.w, n, db ? db : dof, reinterpret_cast<const uint64_t *>(dof),
                                    reinterpret_cast<uint32_t *>(dv), df, s));
            if ((rc = batch_done(ix, ln))) return rc;
            hb.g.unlock();
            HIPCHK(ix, hipStreamSynchronize(s));
            return TM_OK;
        }
    }
    const uint8_t *dbytes;
    const uint64_t *doffs;
    if ((rc = stage_in(ix, ln, n, tb, to, nullptr, dbytes, doffs))) return rc;
    const uint64_t rbytes = n * 5;   // first value u32 per topic, then the found flags
    uint8_t *dres;
    if ((rc = stage_out(ix, ln, n, rbytes, dres))) return rc;
    HIPCHK(ix, launch_first(dev_view(ix, ln.r), ln.w, n, dbytes, doffs, reinterpret_cast<uint32_t *>(dres), dres + n * 4, s));
    if ((rc = fetch_out(ix, ln, n, rbytes))) return rc;
    if ((rc = batch_done(ix, ln))) return rc;
    hb.g.unlock();
    HIPCHK(ix, hipStreamSynchronize(s));
    if (n) {
        memcpy(out_value, ln.pin_out, n * 4);
        memcpy(out_found, ln.pin_out + n * 4, n);
    }
    return TM_OK;
}

int tm_merge_shards(uint32_t world, uint64_t n, const uint64_t *shard_hit, const uint32_t *shard_vals,
                    uint64_t stride, uint64_t *out_hit, uint32_t *out, uint64_t cap, void *stream) {
    if (!world || !shard_hit || !out_hit || (cap && !out) || (n && !shard_vals))
        return fail(nullptr, TM_EINVAL, "tm_merge_shards: bad argument");
    hipError_t e = launch_merge_shards(world, n, shard_hit, shard_vals, stride, out_hit, out, cap,
                                       reinterpret_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(nullptr, TM_EDEVICE, std::string("tm_merge_shards: ") + hipGetErrorString(e));
    return TM_OK;
}

int tm_profile_enable(tm_index *ix, int enable) {
    if (!ix) return fail(nullptr, TM_EINVAL, "tm_profile_enable: null handle");
    std::lock_guard<std::mutex> g(ix->mu);
    ix->prof = enable != 0;
    return TM_OK;
}

int tm_profile_read(tm_index *ix, double *walk_ms, double *batch_ms, uint64_t *batches, int reset) {
    if (!ix) return fail(nullptr, TM_EINVAL, "tm_profile_read: null handle");
    std::lock_guard<std::mutex> g(ix->mu);
    for (auto &ev : ix->prof_pending) {
        HIPCHK(ix, hipEventSynchronize(ev.b1));
        float w = 0, b = 0;
        if (ev.w0) { HIPCHK(ix, hipEventElapsedTime(&w, ev.w0, ev.w1)); }
        HIPCHK(ix, hipEventElapsedTime(&b, ev.b0, ev.b1));
        ix->prof_walk_ms += w; ix->prof_batch_ms += b; ix->prof_batches++;
        ix->prof_free.push_back(ev);
    }
    ix->prof_pending.clear();
    if (walk_ms) *walk_ms = ix->prof_walk_ms;
    if (batch_ms) *batch_ms = ix->prof_batch_ms;
    if (batches) *batches = ix->prof_batches;
    if (reset) { ix->prof_walk_ms = ix->prof_batch_ms = 0; ix->prof_batches = 0; }
    return TM_OK;
}

int tm_debug_set(tm_index *ix, uint32_t key, uint64_t value) {
    if (!ix) return fail(nullptr, TM_EINVAL, "tm_debug_set: null handle");
    std::lock_guard<std::mutex> g(ix->mu);
    switch (key) {
    case TM_DEBUG_LB_SPINS: ix->dbg_lb.spins = value > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)value; break;
    case TM_DEBUG_LB_FAIL_BLOCK: ix->dbg_lb.fail_block = value > 0xFFFFFFFFull ? NONE : (uint32_t)value; break;
    case TM_DEBUG_LB_LAUNCHES: ix->dbg_lb_launches = value; break;
    case TM_DEBUG_PHASES: ix->dbg_phases = value != 0; break;
    case TM_DEBUG_COMBINE: ix->cmb_leaders = value > 16 ? 16 : (int)value; break;
    case TM_DEBUG_CMB_GATHER: ix->cmb_gather_us = value > 1000 ? 1000 : (int)value; break;
    case TM_DEBUG_CMB_LAND: if (value) return fail(ix, TM_EINVAL, "tm_debug_set: TM_DEBUG_CMB_LAND was removed"); break;
    case TM_DEBUG_CMB_SPIN: ix->cmb_spin_us = value > 1000 ? 1000 : (int)value; break;
    case TM_DEBUG_SMALL_TICKET: ix->small_ticket = value != 0; break;
    case TM_DEBUG_PATCH_ZC: ix->patch_zc = value != 0; break;
    case TM_DEBUG_DP1_MAX: ix->dp1_max = std::min<uint64_t>(value, DP1_DELIVERIES); break;
    case TM_DEBUG_GS1_MAX: ix->gs1_max = std::min<uint64_t>(value, GS1_DELIVERIES); break;
    case TM_DEBUG_GP1_MAX: ix->gp1_max = std::min<uint64_t>(value, GP1_DELIVERIES); break;
    case TM_DEBUG_SMALL_KERNEL:
        if (value != SMALL_AUTO && value != SMALL_WAVE && value != SMALL_WAVE8)
            return fail(ix, TM_EINVAL, "tm_debug_set: TM_DEBUG_SMALL_KERNEL is 0, 1 or 3 (2, the lane kernel, was removed)");
        ix->small_kind = (int)value;
        break;
    default: return fail(ix, TM_EINVAL, "tm_debug_set: unknown key");
    }
    return TM_OK;
}

int tm_debug_get(tm_index *ix, uint32_t key, uint64_t *value) {
    if (!ix || !value) return fail(ix, TM_EINVAL, "tm_debug_get: null argument");
    switch (key) {
    case TM_DEBUG_FAILED_BATCHES: *value = ix->failed_batches.load(); break;
    case TM_DEBUG_RETRIED_BATCHES: *value = ix->retried_batches.load(); break;
    case TM_DEBUG_PATH_PHASES: *value = ix->path_batches[PATH_PHASES].load(); break;
    case TM_DEBUG_PATH_SMALL: *value = ix->path_batches[PATH_SMALL].load(); break;
    case TM_DEBUG_PATH_LANE: *value = ix->path_batches[PATH_LANE].load(); break;
    case TM_DEBUG_COMBINE: *value = (uint64_t)ix->cmb_leaders.load(); break;
    case TM_DEBUG_CMB_GATHER: *value = (uint64_t)ix->cmb_gather_us.load(); break;
    case TM_DEBUG_CMB_LAND: *value = 0; break;
    case TM_DEBUG_CMB_SPIN: *value = (uint64_t)ix->cmb_spin_us.load(); break;
    case TM_DEBUG_COMMITS: *value = ix->commits.load(); break;
    case TM_DEBUG_SMALL_TICKET: *value = ix->small_ticket; break;
    case TM_DEBUG_PATCH_ZC: *value = ix->patch_zc; break;
    case TM_DEBUG_FANOUT_GRID: *value = FO_GRID; break;
    case TM_DEBUG_ROUTE_ONE: *value = ix->route_one.load(); break;
    case TM_DEBUG_ROUTE_GRID: *value = ix->route_grid.load(); break;
    case TM_DEBUG_DISPATCH_ONE: *value = ix->dispatch_one.load(); break;
    case TM_DEBUG_DISPATCH_GRID: *value = ix->dispatch_grid.load(); break;
    case TM_DEBUG_PUBLISH_ONE: *value = ix->publish_one.load(); break;
    case TM_DEBUG_PUBLISH_GRID: *value = ix->publish_grid.load(); break;
    case TM_DEBUG_GROUP_TILE: *value = GS_TILE; break;
    case TM_DEBUG_GROUP_GRID: *value = GS_GRID; break;
    case TM_DEBUG_GROUP_PASSES_RUN:
    case TM_DEBUG_GROUP_PASSES_SKIPPED: {
        std::lock_guard<std::mutex> g(ix->mu);
        if (int rc = group_passes(ix, key == TM_DEBUG_GROUP_PASSES_SKIPPED, *value)) return rc;
        *value += ix->gs1_passes[key == TM_DEBUG_GROUP_PASSES_SKIPPED].load();   // (k_gs_one's, counted on the host)
        break;
    }
    case TM_DEBUG_DELIVER_ONE: *value = ix->deliver_one.load(); break;
    case TM_DEBUG_DELIVER_GRID: *value = ix->deliver_grid.load(); break;
    case TM_DEBUG_GS1_MAX: {
        std::lock_guard<std::mutex> g(ix->mu);
        *value = ix->gs1_max;
        break;
    }
    case TM_DEBUG_GP1_MAX: {
        std::lock_guard<std::mutex> g(ix->mu);
        *value = ix->gp1_max;
        break;
    }
    case TM_DEBUG_PUBLISH_DELIVER_ONE: *value = ix->publish_deliver_one.load(); break;
    case TM_DEBUG_PUBLISH_DELIVER_GRID: *value = ix->publish_deliver_grid.load(); break;
    case TM_DEBUG_DP1_MAX: {
        std::lock_guard<std::mutex> g(ix->mu);
        *value = ix->dp1_max;
        break;
    }
    case TM_DEBUG_SUB_COMPACTIONS: {
        std::lock_guard<std::mutex> dg(ix->dst_mu);
        *value = ix->subs_h.compactions;
        break;
    }
    case TM_DEBUG_COMMIT_WAITS: *value = ix->commit_waits.load(); break;
    case TM_DEBUG_COMMIT_FORCED: *value = ix->commit_forced.load(); break;
    case TM_DEBUG_COMBINED_LAUNCHES: *value = ix->cmb_launches.load(); break;
    case TM_DEBUG_COMBINED_BATCHES: *value = ix->cmb_batches.load(); break;
    case TM_DEBUG_WIDE_NODES:
    case TM_DEBUG_DENSE_WIDE: {   // wide nodes / those of them that probe their table without the bitmap
        std::lock_guard<std::mutex> g(ix->img);
        uint64_t v = 0;
        for (uint32_t node : ix->wide) v += key == TM_DEBUG_WIDE_NODES || ix->nodes.h[node].kw[2] == NONE;
        *value = v;
        break;
    }
    case TM_DEBUG_ANNEX0:
    case TM_DEBUG_ANNEX1: {
        std::lock_guard<std::mutex> g(ix->img);
        const uint32_t p = ix->anx[key - TM_DEBUG_ANNEX0];
        *value = p == NONE ? ~0ull : (uint64_t)ix->aux[p].depth << 32 | nlit_of(ix->nodes.h[p]);
        break;
    }
    case TM_DEBUG_HINT_AUDIT: {   // every short word's hint of every annexed node against that node's table
        std::lock_guard<std::mutex> g(ix->img);
        uint64_t bad = 0;
        for (uint32_t s = 0; s < ANX_SLOTS; s++) {
            const uint32_t p = ix->anx[s];
            if (p == NONE) continue;
            const Node &pn = ix->nodes.h[p];
            const uint32_t flag = s ? NLIT_ANX1 : NLIT_ANX0;
            bad += (pn.nlit & (NLIT_ANX0 | NLIT_ANX1)) != flag || nlit_of(pn) < WIDE_LIT;
            for (const VocabEntry &e : ix->vocab.h) {
                if (e.wid == NONE || (e.tag & 0xFFu) > VINL) continue;
                const uint32_t sl = ctab_find(ix, pn.kw[0], pn.kw[1], e.wid);
                const CSlot *c = sl == NONE ? nullptr : &ix->ctab.h[pn.kw[0] + sl];
                bad += ((e.tag >> (s ? HINT_SHIFT1 : HINT_SHIFT0)) & HINT_MASK) != (c ? hint_of_sum(c->sum_lo, c->sum_hi) : 0u);
            }
        }
        for (uint32_t id = 0; id < ix->nodes.h.size(); id++)   // no other line carries a flag
            bad += (ix->nodes.h[id].nlit & (NLIT_ANX0 | NLIT_ANX1)) && annex_slot(ix, id) < 0;
        *value = bad;
        break;
    }
    default: return fail(ix, TM_EINVAL, "tm_debug_get: unknown key");
    }
    return TM_OK;
}

// ------------------------------------------------------- matches_filter/3

}  // extern "C"

namespace {

void mf_words_of(const uint8_t *p, uint32_t n, std::vector<std::string> &out) {
    out.clear();
    uint32_t s0 = 0;
    for (uint32_t i = 0; i <= n; i++)
        if (i == n || p[i] == '/') { out.emplace_back(reinterpret_cast<const char *>(p) + s0, i - s0); s0 = i + 1; }
}

// rank of a word: '#' 0, '+' 1, a binary word 3 + 2 i if it is words[i], else
// 2 + 2 i (i = the words before it): term order (atoms < binaries, bytes)
uint32_t mf_rank(const std::vector<std::string> &words, const std::string &w, bool wild) {
    if (wild) return w == "#" ? 0 : 1;
    const auto it = std::lower_bound(words.begin(), words.end(), w);
    const uint32_t i = (uint32_t)(it - words.begin());
    return it != words.end() && *it == w ? 3 + 2 * i : 2 + 2 * i;
}

// the words of a key (or query) in bytes + flags form: escaped word lists
// decoded, else split on '/' with bare "+" / "#" the wildcards
void mf_key_words(const uint8_t *p, uint32_t n, uint8_t flags, std::vector<std::pair<std::string, bool>> &out) {
    if (flags & TM_KEY_ESCAPED) { esc_words(p, n, out); return; }
    std::vector<std::string> ws;
    mf_words_of(p, n, ws);
    out.clear();
    for (auto &x : ws) out.emplace_back(x, x == "+" || x == "#");
}

void mf_free_keys(tm_index::MfState &m) {
    for (void *p : {(void *)m.pool, (void *)m.koff, (void *)m.val}) if (p) (void)hipFree(p);
    m.pool = nullptr; m.koff = nullptr; m.val = nullptr; m.K = 0; m.pcap = m.kcap = m.vcap = 0;
}

// the filter of trie node `node` (words joined by '/'), for the snapshot
void mf_path(tm_index *ix, uint32_t node, std::string &out) {
    std::vector<uint32_t> up;
    for (uint32_t x = node; x != ROOT; x = ix->aux[x].parent) up.push_back(x);
    out.clear();
    std::string w;
    for (size_t i = up.size(); i-- > 0;) {
        const NodeAux &a = ix->aux[up[i]];
        if (a.is_plus) w = "+";
        else vocab_bytes(ix, ix->vocab.h[ix->wslot[a.wid]], w);
        if (i + 1 != up.size()) out.push_back('/');
        out += w;
    }
}

// Fuzzy snapshot of the word-list keys (caller holds m.mu, not ix->mu): the
// log starts first, then the trie's nodes are read in slices under the image
// lock (ix->img), each ending after MF_SLICE_US (checked every 64 nodes); replaying the
// log afterwards makes the copy exact (a key untouched since the log started
// sits on a node that cannot move, so a slice sees it; any other key ends as
// its last logged op leaves it).
constexpr double MF_SLICE_US = 100.0;

void mf_snapshot(tm_index *ix) {
    auto &m = ix->mf;
    m.keys.clear();
    {
        std::lock_guard<std::mutex> g(ix->img);
        m.log.clear();
        m.log_on = true;
        m.log_lost = false;
        for (const std::string &k : ix->dead) m.keys.insert(k);
    }
    std::string path, key;
    for (uint64_t cur = 0;;) {
        std::lock_guard<std::mutex> g(ix->img);
        const auto t0 = std::chrono::steady_clock::now();
        uint64_t end = ix->nodes.h.size(), x = cur;
        for (; x < end; x++) {
            if ((x & 63) == 63 &&
                std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() > MF_SLICE_US) {
                end = x;
                break;
            }
            const Node &n = ix->nodes.h[x];
            if (!(n.exact_cnt & RUN_CNT) && !(n.hash_cnt & RUN_CNT)) continue;
            mf_path(ix, (uint32_t)x, path);
            const NodeAux &a = ix->aux[x];
            auto add = [&](uint32_t roff, uint32_t cnt, bool hash) {
                for (uint32_t i = 0; i < cnt; i++) {
                    const uint32_t v = ix->vals.h[roff + i];
                    // (the root has no words; a node whose path is one empty word has path "")
                    std::string f = hash ? (x == ROOT ? std::string("#") : path + "/#") : path;
                    m.keys.insert(dead_key(reinterpret_cast<const uint8_t *>(f.data()), (uint32_t)f.size(), v,
                                           TM_KEY_WORDS));
                }
            };
            add(a.exact_roff, n.exact_cnt & RUN_CNT, false);
            add(a.hash_roff, n.hash_cnt & RUN_CNT, true);
        }
        m.slices++;
        cur = end;
        if (cur >= ix->nodes.h.size()) break;
    }
    m.snapshots++;
    m.have_keys = true;
}

// the device's term-ordered key arrays from m.keys (caller holds m.mu only)
int mf_upload(tm_index *ix) {
    auto &m = ix->mf;
    std::vector<std::pair<std::string, bool>> dw;
    std::vector<std::string> sorted;
    std::unordered_set<std::string> distinct;
    for (const std::string &k : m.keys) {
        if ((uint8_t)k[0] & TM_KEY_EMPTY_LIST) continue;
        mf_key_words(reinterpret_cast<const uint8_t *>(k.data()) + 5, (uint32_t)k.size() - 5, (uint8_t)k[0], dw);
        for (auto &x : dw) if (!x.second) distinct.insert(x.first);
    }
    sorted.assign(distinct.begin(), distinct.end());
    std::sort(sorted.begin(), sorted.end());
    std::vector<uint32_t> pool;
    struct K { uint64_t off; uint32_t len, val; };
    std::vector<K> keys;
    keys.reserve(m.keys.size());
    for (const std::string &k : m.keys) {
        uint32_t v;
        memcpy(&v, k.data() + 1, 4);
        const uint64_t off = pool.size();
        if (!((uint8_t)k[0] & TM_KEY_EMPTY_LIST)) {
            mf_key_words(reinterpret_cast<const uint8_t *>(k.data()) + 5, (uint32_t)k.size() - 5, (uint8_t)k[0], dw);
            for (auto &x : dw) pool.push_back(mf_rank(sorted, x.first, x.second));
        }
        keys.push_back(K{off, (uint32_t)(pool.size() - off), v});
    }
    std::sort(keys.begin(), keys.end(), [&](const K &x, const K &y) {
        const uint32_t m2 = std::min(x.len, y.len);
        for (uint32_t i = 0; i < m2; i++)
            if (pool[x.off + i] != pool[y.off + i]) return pool[x.off + i] < pool[y.off + i];
        if (x.len != y.len) return x.len < y.len;
        return x.val < y.val;
    });
    std::vector<uint32_t> spool;
    spool.reserve(pool.size());
    std::vector<uint64_t> koff(keys.size() + 1, 0);
    std::vector<uint32_t> kval(keys.size());
    for (size_t i = 0; i < keys.size(); i++) {
        koff[i] = spool.size();
        spool.insert(spool.end(), pool.begin() + keys[i].off, pool.begin() + keys[i].off + keys[i].len);
        kval[i] = keys[i].val;
    }
    koff[keys.size()] = spool.size();
    // grow-only device arrays (a free would wait for the device), async copies on the mf stream
    auto grow = [&](auto *&p, uint64_t &cap, uint64_t need, size_t elt) -> int {
        if (need <= cap && p) return TM_OK;
        if (p) { HIPCHK(ix, hipStreamSynchronize(m.s)); HIPCHK(ix, hipFree(p)); }
        p = nullptr;
        cap = need + need / 4 + 1024;
        HIPCHK(ix, hipMalloc(reinterpret_cast<void **>(&p), cap * elt));
        return TM_OK;
    };
    int rc;
    if ((rc = grow(m.pool, m.pcap, spool.size(), 4))) return rc;
    if ((rc = grow(m.koff, m.kcap, koff.size(), 8))) return rc;
    if ((rc = grow(m.val, m.vcap, kval.size(), 4))) return rc;
    if (!spool.empty()) HIPCHK(ix, hipMemcpyAsync(m.pool, spool.data(), spool.size() * 4, hipMemcpyHostToDevice, m.s));
    HIPCHK(ix, hipMemcpyAsync(m.koff, koff.data(), koff.size() * 8, hipMemcpyHostToDevice, m.s));
    if (!kval.empty()) HIPCHK(ix, hipMemcpyAsync(m.val, kval.data(), kval.size() * 4, hipMemcpyHostToDevice, m.s));
    HIPCHK(ix, hipStreamSynchronize(m.s));   // the host vectors die here
    m.K = keys.size();
    m.words.swap(sorted);
    m.dev_stale = false;
    return TM_OK;
}

// bring m.keys up to date: a new snapshot when there is none (or its log was
// dropped), else the logged ops since the last call -- the index lock is
// held only to swap the log out
int mf_refresh(tm_index *ix) {
    auto &m = ix->mf;
    std::vector<std::pair<bool, std::string>> log;
    bool lost;
    {
        std::lock_guard<std::mutex> g(ix->img);
        lost = m.log_lost || !m.log_on;
        if (!lost) log.swap(m.log);
    }
    if (lost || !m.have_keys) {
        mf_snapshot(ix);
        std::lock_guard<std::mutex> g(ix->img);
        log.swap(m.log);
        m.dev_stale = true;
    }
    for (auto &op : log) {
        if (op.first) m.keys.insert(op.second); else m.keys.erase(op.second);
    }
    if (!log.empty()) m.dev_stale = true;
    m.nkeys.store(m.keys.size(), std::memory_order_relaxed);
    return m.dev_stale ? mf_upload(ix) : TM_OK;
}

template <class T>
int mf_grow(tm_index *ix, T *&p, uint64_t &cap, uint64_t need) {
    if (need <= cap && p) return TM_OK;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = std::max<uint64_t>(need + need / 2, 1024);
    HIPCHK(ix, hipMalloc(&p, cap * sizeof(T)));
    return TM_OK;
}

}  // namespace

extern "C" {

int tm_matches_filter(tm_index *ix, uint64_t n, const uint8_t *fb, const uint64_t *fo, uint64_t *out_hit_offsets,
                      uint32_t *out_values, uint64_t cap, uint8_t *out_err) {
    return tm_matches_filter_ex(ix, n, fb, fo, nullptr, out_hit_offsets, out_values, cap, out_err);
}

int tm_matches_filter_ex(tm_index *ix, uint64_t n, const uint8_t *fb, const uint64_t *fo, const uint8_t *ff,
                         uint64_t *out_hit_offsets, uint32_t *out_values, uint64_t cap, uint8_t *out_err) {
    if (!ix) return fail(nullptr, TM_EINVAL, "tm_matches_filter: null handle");
    if (!fo || !out_hit_offsets || !out_err || (n && !fb && fo[n] != fo[0]) || (cap && !out_values))
        return fail(ix, TM_EINVAL, "tm_matches_filter: null buffer");
    if (n >= 0xFFFFFFFFull) return fail(ix, TM_EINVAL, "tm_matches_filter: batch too large");
    auto &m = ix->mf;
    std::lock_guard<std::mutex> g(m.mu);   // control plane: one call at a time; the index lock stays free
    HIPCHK(ix, hipSetDevice(ix->rep[0].device));   // matches_filter's arrays live on replica 0
    if (!m.s) HIPCHK(ix, hipStreamCreateWithFlags(&m.s, hipStreamNonBlocking));
    int rc;
    if ((rc = mf_refresh(ix))) return rc;
    // queries: filter_words/1 (:359-366) -> ranks; base_init on a '$' first word
    std::vector<uint32_t> qoff(n + 1, 0), qr, qbase(n, NONE);
    std::vector<std::pair<std::string, bool>> w;
    for (uint64_t i = 0; i < n; i++) {
        mf_key_words(fb + fo[i], (uint32_t)(fo[i + 1] - fo[i]), ff ? ff[i] : 0, w);
        for (auto &x : w) qr.push_back(mf_rank(m.words, x.first, x.second));
        if (!w[0].second && !w[0].first.empty() && w[0].first[0] == '$') qbase[i] = mf_rank(m.words, w[0].first, false);
        qoff[i + 1] = (uint32_t)qr.size();
    }
    const uint64_t qwords = (n + 1) + qr.size() + n + n;   // offsets, ranks, bases, counts
    if ((rc = mf_grow(ix, m.q, m.qcap, qwords))) return rc;
    if ((rc = mf_grow(ix, m.err, m.ecap, n + 1))) return rc;
    if ((rc = mf_grow(ix, m.hit, m.hcap, n + 1))) return rc;
    uint32_t *d_qoff = m.q, *d_qr = m.q + n + 1, *d_qbase = d_qr + qr.size(), *d_cnt = d_qbase + n;
    HIPCHK(ix, hipMemcpyAsync(d_qoff, qoff.data(), (n + 1) * 4, hipMemcpyHostToDevice, m.s));
    if (!qr.empty()) HIPCHK(ix, hipMemcpyAsync(d_qr, qr.data(), qr.size() * 4, hipMemcpyHostToDevice, m.s));
    if (n) HIPCHK(ix, hipMemcpyAsync(d_qbase, qbase.data(), n * 4, hipMemcpyHostToDevice, m.s));
    HIPCHK(ix, hipMemsetAsync(m.err, 0, n + 1, m.s));
    HIPCHK(ix, launch_matches_filter(n, d_qoff, d_qr, d_qbase, m.pool, m.koff, m.val, m.K, d_cnt, nullptr, nullptr,
                                     0, m.err, m.s));
    std::vector<uint32_t> cnt(n);
    if (n) HIPCHK(ix, hipMemcpyAsync(cnt.data(), d_cnt, n * 4, hipMemcpyDeviceToHost, m.s));
    HIPCHK(ix, hipStreamSynchronize(m.s));
    out_hit_offsets[0] = 0;
    for (uint64_t i = 0; i < n; i++) out_hit_offsets[i + 1] = out_hit_offsets[i] + cnt[i];
    const uint64_t total = out_hit_offsets[n];
    if (total && cap) {
        const uint64_t wcap = std::min(total, cap);
        if ((rc = mf_grow(ix, m.out, m.ocap, wcap))) return rc;
        HIPCHK(ix, hipMemcpyAsync(m.hit, out_hit_offsets, (n + 1) * 8, hipMemcpyHostToDevice, m.s));
        HIPCHK(ix, launch_matches_filter(n, d_qoff, d_qr, d_qbase, m.pool, m.koff, m.val, m.K, d_cnt, m.hit, m.out,
                                         wcap, m.err, m.s));
        HIPCHK(ix, hipMemcpyAsync(out_values, m.out, wcap * 4, hipMemcpyDeviceToHost, m.s));
    }
    if (n) HIPCHK(ix, hipMemcpyAsync(out_err, m.err, n, hipMemcpyDeviceToHost, m.s));
    HIPCHK(ix, hipStreamSynchronize(m.s));
    if (total > cap) return fail(ix, TM_ECAP, "tm_matches_filter: output capacity too small");
    return TM_OK;
}

int tm_stats(tm_index *ix, tm_stats_t *o) {
    if (!ix || !o) return fail(ix, TM_EINVAL, "tm_stats: null argument");
    std::lock_guard<std::mutex> g(ix->img);
    memset(o, 0, sizeof *o);
    o->n_wild_keys = ix->n_wild;
    o->n_exact_keys = ix->n_exact;
    o->n_dead_keys = ix->dead.size();
    o->n_keys = ix->n_wild + ix->n_exact + ix->dead.size();
    o->n_nodes = ix->live_nodes;
    o->n_edges = ix->nlinks;
    o->n_words = ix->vcount;
    o->device_bytes = ix->vocab.dcap * sizeof(VocabEntry)   /* per replica */ + ix->wpool.dcap + ix->nodes.dcap * sizeof(Node) +
                      ix->ctab.dcap * sizeof(CSlot) + ix->vals.dcap * 4 + ix->exact.dcap * sizeof(ExactEntry) + ix->xfp.dcap * 2 +
                      ix->wseq.dcap * 4 + ix->wbits.dcap * 4;
    o->uploads = ix->uploads;
    o->patch_bytes = ix->patch_bytes;
    return TM_OK;
}

}  // extern "C"
