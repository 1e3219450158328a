// tm_dev.h -- what the host side hands to the gfx950 kernels (tm_kernels.hip).
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>
#include "tm_layout.h"

namespace tmx {

// Read-only view of the HBM-resident index (one snapshot per batch; patches
// are applied in stream order before the batch's kernels run).
// tm_commit compares two views field by field (tm_host.cpp same_view): a new
// field goes there as well.
struct DevIndex {
    const VocabEntry *vocab; uint32_t vmask;
    const uint8_t *wpool;
    const Node *nodes;
    const CSlot *ctab;
    const uint32_t *vals;
    const ExactEntry *exact; uint32_t xmask;
    const uint16_t *xfp;
    const uint32_t *wseq;
    const uint32_t *wbits; uint32_t wcap;   // wide nodes' child bitmaps, bits per bitmap (tm_layout.h WIDE_LIT)
    // A walk needs a topic's level words only down to the trie's depth (no node
    // deeper than `depth` exists), unless a binary key of the topic's length
    // exists (xlen_mask bit L for L < 64, L <= xlen_max beyond): need_levels().
    uint32_t depth, xlen_max;
    uint64_t xlen_mask;
    uint32_t hdesc;   // keys with a '#' that is not last are stored (NLIT_HDESC nodes exist)
    // depth of the node annexed to each vocab-hint slot (tm_layout.h HINT_*): the
    // walk keeps that slot's hint of its word at this level (NONE: slot unused)
    uint32_t anx_depth[ANX_SLOTS];
};

constexpr int FAST_L = 8;        // levels handled by the main walk kernel (LDS frontier)

// levels of an L-level topic whose words a walk must resolve (see DevIndex)
__host__ __device__ __forceinline__ uint32_t need_levels(const DevIndex &ix, uint32_t L) {
    const bool exact = L < 64 ? ((ix.xlen_mask >> L) & 1u) != 0 : L <= ix.xlen_max;
    return exact || L < ix.depth ? L : ix.depth;
}
constexpr int MID_L = 32;        // levels handled by the list kernels with an LDS frontier
constexpr int MAX_LEVELS = 65536;// MQTT topics are <= 65535 bytes
constexpr int RCAP = 8;          // terminal ranges kept per topic before the re-walk path
constexpr int DEEP_LANES = 64;   // lanes of the global-scratch (deep / overflow) kernels

enum { L_MID = 0, L_DEEP = 1, L_OVF_MID = 2, L_OVF_DEEP = 3, L_COUNT = 4 };

// Per-batch device scratch (grow-only, owned by the index).
// The one-launch kernel's (k_walk_small) look-back word of a
// block: launch tag (19 bits), state (LB_AGG: its own hit total; LB_INCL: the
// total of it and every block before it; LB_FAIL: its wait expired, or a
// predecessor's did -- every later block fails too) and the value (42 bits)
// in ONE 64-bit word, so a reader gets state and value from one coherent load
// (no acquire / release: those write back and invalidate the whole L2 of the
// XCD, under every kernel running there)
enum : uint32_t { LB_AGG = 1, LB_INCL = 2, LB_FAIL = 3 };
constexpr uint32_t LB_TAG_BITS = 19, LB_TAG_MASK = (1u << LB_TAG_BITS) - 1;
constexpr uint64_t LB_VAL_MASK = (1ull << 42) - 1;
__host__ __device__ constexpr uint64_t lb_word(uint32_t tag, uint32_t st, uint64_t v) {
    return (uint64_t)tag << 45 | (uint64_t)st << 42 | (v & LB_VAL_MASK);
}
__host__ __device__ constexpr uint32_t lb_tag(uint64_t w) { return (uint32_t)(w >> 45); }
__host__ __device__ constexpr uint32_t lb_state(uint64_t w) { return (uint32_t)(w >> 42) & 7u; }

// The look-back's bounded wait.  A block waits only for blocks that started
// before it (so they are running and publish soon); the bound keeps a lost
// publication (e.g. a predecessor's waves preempted for long) from leaving a
// spinning grid behind: past it the block and every later one flag their
// topics err 4 and raise the workspace's fail word, and the host API runs the
// batch again (tm_host.cpp HostBatch::run).
constexpr uint32_t LB_SPINS = 1u << 22;   // polls of one predecessor word (LB_SLEEP apart: >= 0.1 s)
constexpr uint32_t LB_SLEEP = 1;          // s_sleep between polls of a word not yet published (x 64 clocks)
constexpr uint32_t LB_STRIDE = 1;         // 8-B words between consecutive blocks' look-back words
struct LbCtl {
    uint32_t spins;        // the bound (LB_SPINS; tm_debug_set can lower it)
    uint32_t fail_block;   // test hook: this block acts as if its wait expired (NONE: off)
    uint32_t ticket;       // 1: k_walk_small's blocks take a start-order ticket (TM_DEBUG_SMALL_TICKET)
};

constexpr int SMALL_SEGS = 16;   // host batches one combined small launch can carry (SmallSegs)

struct Workspace {
    uint32_t *cnt;        // [n] hits per topic
    uint32_t *nr;         // [n] ranges per topic (RCAP+1 = overflow)
    uint2 *rng;           // [n * RCAP] (value offset, count)
    uint32_t *lists;      // [(L_COUNT + 1) * n] topic lists (the last one: long segments to sort)
    uint32_t *list_n;     // [L_COUNT] list lengths, [L_COUNT] reset ticket, [L_COUNT + 1] scan ticket,
                          // [L_COUNT + 2] long-segment count, [L_COUNT + 3] its reset ticket,
                          // [SM_TICK + k] k_walk_small's start-order ticket of segment k (zero between launches)
    uint64_t *blk;        // [n / TILE + 4] tile hit totals (zero between batches)
    uint64_t *sup;        // [n / (TILE * SUP) + 4] superblock hit totals (zero between batches; in blk's allocation)
    uint32_t *deep_wid;   // [DEEP_LANES * MAX_LEVELS]
    uint2 *deep_stk;      // [DEEP_LANES * (MAX_LEVELS + 1)]
    uint8_t *deep_plus;   // [DEEP_LANES * MAX_LEVELS] '+' levels of each deep lane's path
    uint64_t *look;       // [(n / SM_TOPICS + 4) * LB_STRIDE] one-launch kernels: per block, one look-back word (lb_word)
    uint32_t *pairs;      // [2 * SMALL_SEGS] pairs launches: per segment, its values counter and block ticket (zero between launches)
    uint64_t *vres;       // [VRES_WORDS] a device pairs batch's value reservations (zero between batches):
                          // region k's fill at [k * VRES_STRIDE], its failed attempts at [+1]; the pool at [VRES_POOL]
    // list lengths of the last count-mode batch that finished here ([0, L_COUNT))
    // and its topic count ([L_COUNT]; 0: none yet), written by the device into
    // mapped host memory: the next batch sizes its tail grids from them;
    // [HINT_FAIL]: set by a one-launch kernel whose look-back failed (the host
    // clears it)
    uint32_t *hint_h, *hint_d;
    uint64_t cap_n;
};

constexpr int TILE = 256;    // topics per walk block = per scan tile = per emit block
constexpr int SUP = 64;      // tiles per superblock (Workspace::sup)
constexpr int SM_TICK = L_COUNT + 4;     // Workspace::list_n words: k_walk_small's tickets, one per segment
constexpr int LIST_SLOTS = SM_TICK + SMALL_SEGS;   // Workspace::list_n entries
constexpr int HINT_FAIL = L_COUNT + 1;    // Workspace::hint_* word of the fail flag
constexpr int HINT_WORDS = L_COUNT + 2;
// A device pairs batch reserves its values' spans in VRES_K regions of the
// output (a walk block takes region blockIdx % VRES_K, each region's counter on
// a line of its own) and, when its region is full, in the pool at the top: one
// hot counter took 15.6k same-address device-scope atomics per 1M-topic batch,
// +80 us on a 250 us walk
constexpr int VRES_K = 64;
constexpr int VRES_STRIDE = 16;                      // u64 words between counters (128 B)
constexpr int VRES_POOL = VRES_K * VRES_STRIDE;
constexpr int VRES_WORDS = VRES_POOL + VRES_STRIDE;
constexpr int SM_TOPICS = 16;             // topics per block of the one-launch small-batch path
constexpr int SM_TB = 256;                // topic bytes it stages in LDS (longer topics: the lane walk)
constexpr int SM_VSTAGE = 1024;           // values of a block it stages in LDS before one contiguous write


// Pipeline entry points (tm_kernels.hip).  All asynchronous on `s`.
// phase 1: tokenise + walk + tile totals (hit_offs[n] = total becomes valid)
// phase 2: finish the scan (hit_offs[0..n)), emit the values, re-walk
//          overflowing topics, reset the device-side list counters
// ev_walk0/ev_walk1 (may be null): recorded right before / after the main walk kernel
hipError_t launch_match_phase1(const DevIndex &ix, const Workspace &ws, uint64_t n, const uint8_t *bytes,
                               const uint64_t *offs, uint64_t *hit_offs, uint8_t *err, hipStream_t s,
                               hipEvent_t ev_walk0 = nullptr, hipEvent_t ev_walk1 = nullptr);
hipError_t launch_match_phase2(const DevIndex &ix, const Workspace &ws, uint64_t n, const uint8_t *bytes,
                               const uint64_t *offs, uint64_t *hit_offs, uint32_t *out, uint64_t cap,
                               hipStream_t s);
// A batch with its hit lists as per-topic (first position, count) pairs
// (pairs[2 t], pairs[2 t + 1]; pairs[2 n] = the values' total, saturated at
// 2^32 - 1): k_walk_pairs writes every value itself, k_tail_pairs finishes the
// deep and overflowed topics -- two launches, no scan and no k_emit
hipError_t launch_match_pairs(const DevIndex &ix, const Workspace &ws, uint64_t n, const uint8_t *bytes,
                              const uint64_t *offs, uint8_t *err, uint32_t *pairs, uint32_t *out, uint64_t cap,
                              hipStream_t s, hipEvent_t ev_walk0 = nullptr, hipEvent_t ev_walk1 = nullptr);
// The whole batch in ONE launch when the index allows it: up to SMALL_TOPICS
// topics (small_path_ok: the fallback store of k_walk_small holds the index's
// depth) on k_walk_small (16 or 8 lanes per topic); the two phases otherwise
// (or when `phases` forces them: tests of that path).  `tag` must differ
// between consecutive launches on one workspace (the one-launch look-back scan
// tells its own blocks' words from older ones by it).  A one-launch batch whose
// look-back failed flags its topics err 4 and sets ws.hint_h[HINT_FAIL].
bool small_path_ok(const DevIndex &ix, uint64_t n);
bool one_launch_ok(const DevIndex &ix);
bool lite_path_ok(const DevIndex &ix);   // k_walk_small<8>'s LITE fallback store holds every topic
// which one-launch kernel (small_kind): the default, k_walk_small with 16 / 8
// lanes per topic.  (2 named round 5's k_walk_lane, removed in round 6.)
enum { SMALL_AUTO = 0, SMALL_WAVE = 1, SMALL_WAVE8 = 3 };
enum { PATH_PHASES = 0, PATH_SMALL = 1, PATH_LANE = 2, PATH_COUNT = 3 };   // *path of launch_match (PATH_LANE: retired, 0)
hipError_t launch_match(const DevIndex &ix, const Workspace &ws, uint64_t n, const uint8_t *bytes,
                        const uint64_t *offs, uint64_t *hit_offs, uint8_t *err, uint32_t *out, uint64_t cap,
                        uint32_t tag, LbCtl lb, bool phases, int small_kind, hipStream_t s,
                        hipEvent_t ev_walk0 = nullptr, hipEvent_t ev_walk1 = nullptr, int *path = nullptr);
// Several host batches in ONE one-launch small kernel (the host's combiner,
// tm_host.cpp small_combined): segment k owns the launch's blocks
// [block0, next block0), its own inputs and outputs and its own look-back
// region; a launch holds at most SMALL_SEGS
// segments of at most SMALL_TOPICS topics together.  Offsets are uint64_t or
// uint32_t for the whole launch.
struct SmallSeg {
    const uint8_t *blob; const void *offs; void *hit; uint8_t *err; uint32_t *out;
    uint64_t cap; uint32_t n, block0;
};
// pairs: the launch writes per-topic (first position, count) pairs instead of
// a CSR (hit[2 t], hit[2 t + 1]; hit[2 n] = the values' total; u32 offsets
// only): tm_match_batch32_pairs
struct SmallSegs { uint32_t count, pairs; SmallSeg s[SMALL_SEGS]; };
hipError_t launch_small_segs(const DevIndex &ix, const Workspace &ws, const SmallSegs &sg, bool u32, uint32_t tag,
                             LbCtl lb, int small_kind, hipStream_t s, int *path = nullptr);
// The one-launch small batch with 32-bit offsets in and out (hipErrorInvalidValue
// if small_path_ok refuses the batch), and the 32 <-> 64-bit offset copies
hipError_t launch_match32(const DevIndex &ix, const Workspace &ws, uint64_t n, const uint8_t *bytes,
                          const uint32_t *offs, uint32_t *hit_offs, uint8_t *err, uint32_t *out, uint64_t cap,
                          uint32_t tag, LbCtl lb, int small_kind, hipStream_t s, int *path = nullptr);
hipError_t launch_offs_widen(const uint32_t *in, uint64_t *out, uint64_t m, hipStream_t s);
hipError_t launch_offs_narrow(const uint64_t *in, uint32_t *out, uint64_t m, hipStream_t s);
hipError_t launch_first(const DevIndex &ix, const Workspace &ws, uint64_t n, const uint8_t *bytes,
                        const uint64_t *offs, uint32_t *out_value, uint8_t *out_found, hipStream_t s);
// filter-sharded merge of allgathered per-shard CSR hit lists (k_merge_shards)
hipError_t launch_merge_shards(uint32_t world, uint64_t n, const uint64_t *shard_hit, const uint32_t *shard_vals,
                               uint64_t stride, uint64_t *out_hit, uint32_t *out, uint64_t cap, hipStream_t s);
// sort each topic's segment of a CSR in place (ascending u32); unique: distinct
// values first, padded with 0xFFFFFFFF, distinct count in ucnt (may be null)
hipError_t launch_sort_segments(const Workspace &ws, uint64_t n, const uint64_t *hit_offs, uint32_t *out, uint64_t cap,
                                int unique, uint32_t *ucnt, hipStream_t s);
// out[0 .. min(hit[n], cap)) = src[...] (device -> device or mapped host memory)
hipError_t launch_copy_values(const uint64_t *hit_offs, uint64_t n, const uint32_t *src, uint32_t *dst, uint64_t cap,
                              hipStream_t s);
// Route fan-out (tm_fanout.hip): the CSR's (topic, value) entries at positions
// below min(hit[n], cap), stably partitioned by bucket = dest_of[value] (bucket
// n_dests: v >= dest_len or dest_of[v] >= n_dests) into out_topic / out_value,
// bucket b at [dest_offsets[b], dest_offsets[b + 1]), dest_offsets[n_dests + 1]
// the total.  A fixed grid of FO_GRID one-wave blocks; digits of up to
// FO_MAX_BITS bits; one pass for n_dests + 1 <= 256 buckets, else two through
// the scratch's triples (fs.cap >= min(cap, 2^32 - 1) entries then).
constexpr int FO_GRID = 4096;
constexpr int FO_MAX_BITS = 9;                 // 65537 buckets: 17 bits, 9 + 8
constexpr int FO_BINS = 1 << FO_MAX_BITS;
constexpr uint32_t FO_MAX_DESTS = 65536;
struct FanoutScratch {
    uint32_t *tab;        // [FO_BINS * FO_GRID] per (bin, block) counts, then their scan per bin
    uint32_t *tot;        // [FO_BINS] the bins' totals
    uint32_t *t, *v, *b;  // [cap] a first of two passes' (topic, value, bucket); the pairs form's resolved entries
    uint64_t cap;
    // the pairs form only (launch_fanout_pairs)
    uint64_t *voff;       // [voff_cap] the offsets of the CSR the spans stand for (n + 1 used)
    uint64_t voff_cap;
    uint64_t *sums;       // [FP_TILES] the topic tiles' entry counts
    uint32_t *b2;         // [cap] two passes: the resolved entries' buckets (their topics and values wait in the outputs)
    // aggre (launch_aggre): a bitmap word and a base per 64 positions below ag_cap, the FO_GRID block counts + their total
    uint64_t *ag_bits;
    uint32_t *ag_pre, *ag_cnt;
    uint64_t ag_cap;
    // dispatch (launch_dispatch): the per-entry list lengths below dp_cap, their scan when the caller
    // takes no offsets (dp_off_cap + 1 words), the FO_GRID chunk sums + their total
    uint32_t *dp_cnt;
    uint64_t *dp_off, *dp_tot;
    uint64_t dp_cap, dp_off_cap;
    // shared-subscription pick (launch_share_pick; tab and tot above carry its digit passes): per entry
    // below sh_cap the slot of a ranked entry, two (slot, q) pair arrays for the passes' ping-pong, the
    // FO_GRID ranked / with-slot / picked block counts (3 * FO_GRID + 1 words)
    uint32_t *sh_key, *sh_s[2], *sh_q[2], *sh_cnt;
    uint64_t sh_cap;
    // grouping by subscriber (launch_group_subs): the fixed words (GS_FIX_WORDS: the counters, the plan,
    // the histograms) and, per delivery below gs_cap, the two (key, position) pair arrays of the passes'
    // ping-pong (gs_k[b], gs_p[b]: 16 bytes in all)
    uint32_t *gs_fix, *gs_k[2], *gs_p[2];
    uint64_t gs_cap;
    // picks merged with the deliveries (launch_group_picks; the grouping's scratch above carries its two
    // sorts): one allocation -- GP_FIX_WORDS fixed words, the merged (topic, value, sub, src) arrays below
    // gp_cap (cap + ecap), the local picks' compacted (topic, value, sub) below gp_ecap
    uint32_t *gp_fix, *gp_m[4], *gp_c[3];
    uint64_t gp_cap, gp_ecap;
};
constexpr uint32_t FP_TILES = 1024;
#if defined(__HIPCC__)
// "Which segment holds position p": the device helpers of the fan-out's first
// pass (tm_fanout.hip), shared with the dispatch's expansion (tm_dispatch.hip),
// for one-wave blocks.
// The topic of position p: the last t with hit[t] <= p, i.e. (the first index u
// of [lo, n] with hit[u] > p) - 1, found by the whole wave, 64 probes a round
// (1M offsets: 4 rounds instead of a binary search's 20 dependent loads).
// `lo` is a known lower bound of u.  Reads hit[0 .. n] only, and ends whatever
// the offsets hold.
__device__ __forceinline__ uint64_t fo_topic_at(const uint64_t *hit, uint64_t n, uint64_t p, uint64_t lo,
                                                uint32_t lane) {
    uint64_t hi = n + 1;
    if (lo > hi) lo = hi;
    while (lo < hi) {
        const uint64_t step = (hi - lo + 63) / 64;
        const uint64_t idx = lo + lane * step;
        const bool in = idx < hi;
        const bool gt = in && hit[idx] > p;
        const uint64_t m_gt = __ballot(gt), m_in = __ballot(in);
        if (!m_gt) {
            lo = lo + ((uint64_t)__popcll(m_in) - 1) * step + 1;   // every probe <= p
        } else {
            const uint64_t f = (uint64_t)__builtin_ctzll(m_gt);
            hi = lo + f * step;
            if (f) lo = lo + (f - 1) * step + 1;
        }
    }
    return lo ? lo - 1 : 0;
}

// The topics of one step's positions p0 + lane (`ok`: below the chunk's end c1),
// by the whole wave: a window of the next 64 offsets in LDS that each lane
// searches; lanes whose topic lies beyond it (a run of more than 64 empty
// topics) search again from the first of them.  tcur: hit[tcur] <= p0 on entry,
// the step's last topic on return.
__device__ __forceinline__ uint32_t fo_step_topics(const uint64_t *hit, uint64_t n, uint64_t p0, uint64_t c1, bool ok,
                                                   uint64_t &tcur, uint64_t *s_win, uint32_t lane) {
    const uint64_t p = p0 + lane;
    uint32_t t = 0;
    bool found = !ok;
    uint64_t tw = tcur;
    for (;;) {
        // the ends of topics tw .. tw + 63; a lane's topic is tw + (how many of them are <= p)
        const uint64_t idx = tw + 1 + lane;
        s_win[lane] = idx <= n ? hit[idx] : ~0ull;
        __syncthreads();
        if (!found && s_win[63] > p) {
            uint32_t c = 0;
#pragma unroll
            for (uint32_t st = 32; st; st >>= 1)
                if (s_win[c + st - 1] <= p) c += st;
            t = (uint32_t)(tw + c);
            found = true;
        }
        __syncthreads();
        const uint64_t left = __ballot(!found);
        if (!left) break;
        // a run of empty topics longer than the window: search again for the first lane left
        const uint32_t fl = (uint32_t)__builtin_ctzll(left);
        tw = fo_topic_at(hit, n, p0 + fl, tw + 65, lane);
    }
    const uint32_t last = c1 - p0 < 64 ? (uint32_t)(c1 - p0) - 1 : 63u;
    tcur = __shfl(t, last, 64);
    return t;
}
#endif   // __HIPCC__

bool fanout_two_pass(uint32_t n_dests);
hipError_t launch_fanout(const FanoutScratch &fs, uint64_t n, const uint64_t *hit, const uint32_t *values,
                         uint64_t cap, const uint32_t *dest_of, uint64_t dest_len, uint32_t n_dests,
                         uint64_t *dest_offsets, uint32_t *out_topic, uint32_t *out_value, hipStream_t s);
// The same for per-topic (first position, count) pairs (u32, 8-byte aligned,
// [0, 2 n) read): topic t's entries are values[pos_t .. pos_t + eff_t), eff_t =
// min(cnt_t, cap - pos_t) or 0 for pos_t >= cap, in topic order.  Needs
// fs.cap >= min(cap, 2^32 - 1), fs.voff_cap >= n + 1, fs.sums, and fs.b2 for
// two passes.
hipError_t launch_fanout_pairs(const FanoutScratch &fs, uint64_t n, const uint32_t *pairs, const uint32_t *values,
                               uint64_t cap, const uint32_t *dest_of, uint64_t dest_len, uint32_t n_dests,
                               uint64_t *dest_offsets, uint32_t *out_topic, uint32_t *out_value, hipStream_t s);
// A micro-batch's fan-out in ONE launch of ONE workgroup (k_fo_one;
// tm_route_batch32): launch_fanout_pairs' definition with `vcap` bounding the
// spans (eff_t = min(cnt_t, vcap - pos_t)) and `cap` only what is stored --
// entries whose slot is >= cap are counted in dest_offsets but not written.
// dest_offsets (u32[n_dests + 2]), out_topic and out_value may be mapped host
// memory.  status[FO1_ST_STATE] = FO1_DONE, or FO1_TOO_LARGE when n >
// FO1_TOPICS, n_dests + 1 > 256 or the spans hold more than FO1_ENTRIES
// entries: nothing but the status words is written then, and the caller takes
// launch_fanout_pairs.  status[FO1_ST_TOTAL] = pairs[2 n] either way (0 for
// n == 0): the matcher's total, for the caller's capacity checks.
constexpr uint32_t FO1_TOPICS = 8192;
constexpr uint32_t FO1_ENTRIES = 16384;
constexpr uint32_t FO1_BLOCK = 1024;
constexpr uint32_t FO1_MAX_DESTS = 255;        // n_dests + 1 <= 256 buckets: one digit
enum { FO1_ST_STATE = 0, FO1_ST_TOTAL = 1, FO1_ST_WORDS = 2 };
enum : uint32_t { FO1_DONE = 1, FO1_TOO_LARGE = 2 };
hipError_t launch_fanout_one(uint64_t n, const uint32_t *pairs, const uint32_t *values, uint64_t vcap,
                             const uint32_t *dest_of, uint64_t dest_len, uint32_t n_dests, uint32_t *dest_offsets,
                             uint32_t *out_topic, uint32_t *out_value, uint64_t cap, uint32_t *status, hipStream_t s);
// aggre/1 on a fan-out's output (tm_aggre.hip): the entries below E =
// min(dest_offsets[n_dests + 1], cap) without those whose predecessor in the
// same bucket (the unrouted bucket excepted) has the same topic and the same
// filter (filter_of[value] for value < filter_len, else none: equal to
// nothing), in input order, with the kept entries' bucket bounds and the total
// in out_dest_offsets[n_dests + 2].  Needs fs.ag_cap >= min(cap, 2^32 - 1).
// The outputs must not overlap the inputs.
hipError_t launch_aggre(const FanoutScratch &fs, uint32_t n_dests, const uint64_t *dest_offsets, const uint32_t *in_topic,
                        const uint32_t *in_value, uint64_t cap, const uint32_t *filter_of, uint64_t filter_len,
                        uint64_t *out_dest_offsets, uint32_t *out_topic, uint32_t *out_value, hipStream_t s);
// The same for what launch_fanout_one left in device memory (u32 offsets, the
// entries, its status words), in ONE workgroup, into buffers that may be
// mapped host memory.  status_in[FO1_ST_STATE] != FO1_DONE is passed on to
// `status` and nothing else is written; more than `cap` entries before the
// compaction: out_dest_offsets = dest_offsets, no entry written.
hipError_t launch_aggre_one(const uint32_t *status_in, const uint32_t *dest_offsets, uint32_t n_dests,
                            const uint32_t *in_topic, const uint32_t *in_value, const uint32_t *filter_of,
                            uint64_t filter_len, uint32_t *out_dest_offsets, uint32_t *out_topic, uint32_t *out_value,
                            uint64_t cap, uint32_t *status, hipStream_t s);
// Local dispatch (tm_dispatch.hip): bucket `bucket` of a fan-out's or an aggre
// pass's output -- the M entries [q0, q1), q = min(dest_offsets[bucket (+ 1)],
// E), E = min(dest_offsets[n_dests + 1], cap) -- expanded to one delivery per
// (entry, subscriber of the entry's value): span[2 v], span[2 v + 1] = the
// position and length of v's list in pool (v >= span_len, or a span that does
// not lie inside pool_len: no subscribers).  head = [M, T]; the first min(T,
// out_cap) deliveries, in entry order and list order, go to out_topic /
// out_value / out_sub; out_offsets (NULL: fs.dp_off) takes the M + 1 delivery
// offsets.  span must be 8-byte aligned.  Needs fs.dp_cap >= min(cap, 2^32 -
// 1), and fs.dp_off_cap as much when out_offsets is NULL.
hipError_t launch_dispatch(const FanoutScratch &fs, uint32_t n_dests, const uint64_t *dest_offsets, uint32_t bucket,
                           const uint32_t *in_topic, const uint32_t *in_value, uint64_t cap, const uint32_t *span,
                           uint64_t span_len, const uint32_t *pool, uint64_t pool_len, uint64_t *head,
                           uint64_t *out_offsets, uint32_t *out_topic, uint32_t *out_value, uint32_t *out_sub,
                           uint64_t out_cap, hipStream_t s);
// A micro-batch's route outputs and local dispatch in ONE launch of ONE
// workgroup (k_dp_one; tm_dispatch_batch32), from what launch_fanout_one left in
// device memory (fo_*: u32 offsets, the entries, its status words) and, when
// ag_offsets is given, what launch_aggre_one made of it (ag_*; status_in is
// that launch's then).  Writes the caller's route outputs as
// tm_route_batch32_ex defines them (under aggre with more than `cap`
// un-aggregated entries: the fan-out's offsets, no entry), out_head = [M, T]
// of bucket `bucket` of the final arrays with the subscriber table given
// (launch_dispatch's definition), and the first min(T, dcap) deliveries; every
// output may be mapped host memory, none is read.  status[FO1_ST_STATE] =
// FO1_DONE; DP1_TOO_LARGE when T > min(dp1_max, DP1_DELIVERIES): everything
// but the deliveries is written, and the caller takes launch_dispatch on the
// same arrays; a status_in that is not FO1_DONE is passed on and nothing else
// is written.  status[FO1_ST_TOTAL] as launch_fanout_one;
// status[DP1_ST_T_LO / _HI] = T.  span and out_head must be 8-byte aligned.
// (DP1_DELIVERIES: where the one workgroup stops winning against the grid
// kernels' second run, measured host to host: DESIGN.md 4e)
constexpr uint64_t DP1_DELIVERIES = 32768;
enum { DP1_ST_T_LO = FO1_ST_WORDS, DP1_ST_T_HI = FO1_ST_WORDS + 1, DP1_ST_WORDS = FO1_ST_WORDS + 2 };
enum : uint32_t { DP1_TOO_LARGE = 3 };
hipError_t launch_dispatch_one(const uint32_t *status_in, const uint32_t *fo_offsets, const uint32_t *fo_topic,
                               const uint32_t *fo_value, const uint32_t *ag_offsets, const uint32_t *ag_topic,
                               const uint32_t *ag_value, uint32_t n_dests, uint32_t bucket, const uint32_t *span,
                               uint64_t span_len, const uint32_t *pool, uint64_t pool_len, uint32_t *out_dest_offsets,
                               uint32_t *out_topic, uint32_t *out_value, uint64_t cap, uint64_t *out_head,
                               uint32_t *out_dtopic, uint32_t *out_dvalue, uint32_t *out_dsub, uint64_t dcap,
                               uint64_t dp1_max, uint32_t *status, hipStream_t s);
// Shared-subscription pick (tm_share.hip; include/tmatch.h tm_share_pick_dev has
// the definition): one member per entry below E = min(dest_offsets[n_dests + 1],
// cap) of an aggre pass's output into out_member, head = [entries with a slot,
// entries with a pick], the slots' state words advanced once.  slot_rec must be
// 16-byte aligned.  Needs fs.sh_cap >= min(cap, 2^32 - 1), fs.tab and fs.tot.
// The strategy byte of a slot record's meta word (tmatch.h TM_SHARE_*):
enum : uint32_t { SH_RANDOM = 0, SH_ROUND_ROBIN = 1, SH_ROUND_ROBIN_PER_GROUP = 2, SH_STICKY = 3, SH_LOCAL = 4,
                  SH_HASH_CLIENTID = 5, SH_HASH_TOPIC = 6, SH_STRATEGIES = 7 };
uint32_t share_passes(uint64_t n_slots);   // digit passes a call with that many slots runs
hipError_t launch_share_pick(const FanoutScratch &fs, uint32_t n_dests, const uint64_t *dest_offsets,
                             const uint32_t *in_topic, const uint32_t *in_value, uint64_t cap, const uint32_t *key_clientid,
                             const uint32_t *key_topic, uint64_t n_topics, uint32_t seed, const uint32_t *slot_of,
                             uint64_t slot_of_len, const uint32_t *slot_rec, uint64_t n_slots, const uint32_t *pool,
                             uint64_t pool_len, uint32_t *state, uint64_t *head, uint32_t *out_member, hipStream_t s);
// A micro-batch's pick in ONE launch of ONE workgroup (k_sh_one;
// tm_publish_batch32): launch_share_pick's definition over what
// launch_aggre_one left in device memory (u32 offsets, the K <= FO1_ENTRIES
// kept entries, its status words), out_member[0 .. K) into a buffer that may be
// mapped host memory and is never read.  The kernel gates itself, since the
// run that queued it may be run again: it picks and moves state only if
// status_in[FO1_ST_STATE] == FO1_DONE, status_in[FO1_ST_TOTAL] <= vcap and <=
// cap, and *fail (the lane's look-back fail word; may be null) is 0; else it
// writes status[SH1_ST_STATE] = SH1_SKIPPED and nothing else.  Picked:
// status[SH1_ST_HEAD ..] = the head as two u64 (launch_share_pick's), then
// status[SH1_ST_STATE] = SH1_PICKED.  status may be mapped host memory
// (SH1_ST_WORDS words, SH1_ST_HEAD 8-byte aligned).  slot_rec must be 16-byte
// aligned.  No scratch: the ranks come from a stable sort inside LDS.
enum { SH1_ST_STATE = 0, SH1_ST_HEAD = 2, SH1_ST_WORDS = 6 };
enum : uint32_t { SH1_PICKED = 1, SH1_SKIPPED = 2 };
hipError_t launch_share_one(const uint32_t *status_in, const uint32_t *fail, const uint32_t *dest_offsets, uint32_t n_dests,
                            const uint32_t *in_topic, const uint32_t *in_value, uint64_t vcap, uint64_t cap,
                            const uint32_t *key_clientid, const uint32_t *key_topic, uint64_t n_topics, uint32_t seed,
                            const uint32_t *slot_of, uint64_t slot_of_len, const uint32_t *slot_rec, uint64_t n_slots,
                            const uint32_t *pool, uint64_t pool_len, uint32_t *state, uint32_t *out_member, uint32_t *status,
                            hipStream_t s);
// Deliveries grouped by subscriber (tm_group.hip; include/tmatch.h
// tm_group_subs_dev has the definition): the first W = min(head[1], cap)
// deliveries (topic, value, sub) a dispatch wrote, stably sorted by sub into
// out_topic / out_value / out_sub (out_perm, when given: the input positions),
// the G distinct subscribers and their G + 1 offsets -- the first min(G, gcap)
// of them -- into out_gsub / out_goff, ghead = [G, W].  head, ghead and
// out_goff must be 8-byte aligned.  Needs fs.gs_fix and fs.gs_cap >= min(cap,
// 2^32 - 1).  A fixed grid of GS_GRID blocks of GS_BLOCK threads, a block
// ranking GS_TILE keys at a time.
constexpr uint32_t GS_GRID = 1024;
constexpr uint32_t GS_BLOCK = 256;
constexpr uint32_t GS_TILE = 1024;
constexpr uint32_t GS_BINS = 256;                       // 8-bit digits, four passes at most
constexpr uint32_t GS_PASSES = 4;
// fs.gs_fix, in u32 words: the passes run / skipped so far (two u64, zero when allocated), the plan of
// the call in flight (GS_SKIP + p: pass p is the identity; GS_SRC + p: where pass p reads, GS_SRC + 4:
// where the sorted pairs are -- GS_IN the caller's array with positions 0, 1, .., else pair array 0 / 1),
// the head counts of the GS_GRID * 4 waves, the four digits' bin totals (zero between calls), the
// bins' first positions per digit, and the (bin, block) histogram of a pass
enum { GS_STAT = 0, GS_SKIP = 4, GS_SRC = 8, GS_GCNT = 16, GS_TOT = GS_GCNT + GS_GRID * 4,
       GS_BASE = GS_TOT + GS_PASSES * GS_BINS, GS_TAB = GS_BASE + GS_PASSES * GS_BINS,
       GS_FIX_WORDS = GS_TAB + GS_BINS * GS_GRID, GS_ZERO_WORDS = GS_BASE /* zero when allocated */ };
enum : uint32_t { GS_IN = 2 };
hipError_t launch_group_subs(const FanoutScratch &fs, const uint64_t *head, const uint32_t *in_topic,
                             const uint32_t *in_value, const uint32_t *in_sub, uint64_t cap, uint64_t *ghead,
                             uint32_t *out_gsub, uint64_t *out_goff, uint64_t gcap, uint32_t *out_topic,
                             uint32_t *out_value, uint32_t *out_sub, uint32_t *out_perm, hipStream_t s);
// The shared-subscription picks merged with the deliveries and grouped
// (tm_group.hip; include/tmatch.h tm_group_picks_dev has the definition): the
// first W = min(head[1], cap) deliveries a dispatch wrote (ascending topic
// index) and, of the first E = min(dest_offsets[n_dests + 1], ecap) aggregated
// entries, those whose picked member is a local subscriber (sub_of[member]
// != NONE), merged by topic index and stably sorted by subscriber.  ghead =
// [G, N], N = W + P; the first min(N, out_cap) merged deliveries are written,
// out_src (when given) naming a delivery (< W) or W + the pick's rank.  Needs
// fs.gs_fix, fs.gs_cap >= cap + ecap, fs.gp_cap >= cap + ecap, fs.gp_ecap >=
// ecap (both clamped to 2^32 - 1, their sum too: the caller checks).
// msg_passes: every topic index is below 2^(8 * msg_passes) (GS_PASSES: no
// bound known) -- the picks' sort by message queues that many digit passes.
// fs.gp_fix, in u32 words: the picks' head [0, P] and the merged head [0, N]
// (two u64 each, written on the device), the blocks' local-pick counts.
enum { GP_PH = 0, GP_MH = 4, GP_CNT = 8, GP_FIX_WORDS = GP_CNT + GS_GRID };
hipError_t launch_group_picks(const FanoutScratch &fs, const uint64_t *head, const uint32_t *in_topic,
                              const uint32_t *in_value, const uint32_t *in_sub, uint64_t cap, uint32_t n_dests,
                              const uint64_t *dest_offsets, const uint32_t *e_topic, const uint32_t *e_value,
                              const uint32_t *member, uint64_t ecap, const uint32_t *sub_of, uint64_t sub_of_len,
                              uint64_t *ghead, uint32_t *out_gsub, uint64_t *out_goff, uint64_t gcap, uint32_t *out_topic,
                              uint32_t *out_value, uint32_t *out_sub, uint32_t *out_src, uint64_t out_cap,
                              uint32_t msg_passes, hipStream_t s);
// A micro-batch's grouping in ONE launch of ONE workgroup (k_gs_one;
// tm_deliver_batch32), queued behind launch_dispatch_one, which is then given
// the lane's delivery arrays (in_topic / in_value / in_sub, GS1_DELIVERIES
// words each), `head` (two u64 in device memory) for its out_head, and
// min(dp1_max, GS1_DELIVERIES) for its dp1_max.  status_in: the status block
// launch_dispatch_one itself was given (device memory).  With FO1_DONE there
// the kernel passes head = [M, T] on to out_head and, when T <= dp1_max (the
// dispatch expanded), writes launch_group_subs' results over the first W =
// min(T, dcap) deliveries: the grouped arrays, out_ghead = [G, W], the first
// min(G, gcap) subscribers and offsets with the end entry -- out_goff as u32.
// Every output may be mapped host memory, none is read.  status (may be
// mapped host memory): [GS1_ST_STATE] = GS1_GROUPED with the digit passes run
// and skipped and G beside it, or GS1_SKIPPED and nothing else (the caller
// takes the grid kernels).  The kernel moves no state and keeps none: a run queued again
// writes the same outputs again.  head, out_head and out_ghead must be 8-byte
// aligned.  No scratch: a stable sort of 16-bit positions inside LDS, which
// is why one workgroup stops at 16384 deliveries and not at DP1_DELIVERIES.
constexpr uint32_t GS1_DELIVERIES = 16384;
enum { GS1_ST_STATE = 0, GS1_ST_RUN = 1, GS1_ST_SKIPPED = 2, GS1_ST_G = 3, GS1_ST_WORDS = 4 };
enum : uint32_t { GS1_GROUPED = 1, GS1_SKIPPED = 2 };
hipError_t launch_group_one(const uint32_t *status_in, const uint64_t *head, const uint32_t *in_topic,
                            const uint32_t *in_value, const uint32_t *in_sub, uint64_t dcap, uint64_t dp1_max,
                            uint64_t *out_head, uint32_t *out_dtopic, uint32_t *out_dvalue, uint32_t *out_dsub,
                            uint64_t *out_ghead, uint32_t *out_gsub, uint32_t *out_goff, uint64_t gcap, uint32_t *status,
                            hipStream_t s);
// A micro-batch's picks merged with its deliveries and grouped in ONE launch
// of ONE workgroup (k_gp_one; tm_publish_deliver_batch32), queued behind
// launch_dispatch_one (given the lane's delivery arrays and `head`, as under
// launch_group_one), launch_pd_gate and launch_share_one.
// launch_pd_gate (k_pd_gate, one wave) decides ONCE, on the device, whether the
// run that queued the three stands and fits one workgroup, and writes that into
// `gate` (one device word: 0 go, else skip), which launch_share_one is given as
// its fail word and launch_group_picks_one reads: the pick is made and the state
// moves exactly when the merge and the grouping run.  status_in: the block
// launch_dispatch_one itself was given; head: the [M, T] it left on the lane;
// dest_offsets: the aggre pass's u32 offsets (K = dest_offsets[n_dests + 1]);
// fail: the lane's look-back fail word (may be null).  With FO1_DONE in
// status_in out_head = head (mapped host memory).  Go needs launch_share_one's
// own conditions (FO1_DONE, total <= vcap, total <= cap, *fail == 0, n_dests <=
// FO1_MAX_DESTS) and T <= tmax, T + K <= min(dcap, nmax); tmax and nmax are
// clamped to GP1_DELIVERIES.  status (may be mapped host memory):
// [PD1_ST_STATE] = PD1_GO or PD1_SKIP, [PD1_ST_REASON] = the first condition
// in the order of PD1_R_* that failed, [PD1_ST_T] / [PD1_ST_K] = T (saturated)
// and K where status_in was FO1_DONE.
// launch_group_picks_one: a non-zero gate word gives status[GP1_ST_STATE] =
// GP1_SKIPPED and nothing else.  Otherwise member[0 .. K) (what
// launch_share_one wrote on the lane) goes to out_member, and
// launch_group_picks' results over the T deliveries and the K entries with
// sub_of (sub_of_len words) go to the caller's buffers: the N = T + P merged
// and grouped deliveries below dcap, out_ghead = [G, N], the first min(G, gcap)
// subscribers and offsets with the end entry -- out_goff as u32.  Every output
// may be mapped host memory, none is read.  status: [GP1_ST_STATE] =
// GP1_GROUPED with the digit passes run and skipped (of GS_PASSES for each of
// the two sorts), G, P and N beside it.  head and out_ghead must be 8-byte
// aligned.  No scratch: both sorts run over 16-bit codes inside LDS; a pick's
// message and entry position are staged there too, which is why one workgroup
// stops at 8192 merged deliveries where k_gs_one takes 16384.
constexpr uint32_t GP1_DELIVERIES = 8192;
enum { PD1_ST_STATE = 0, PD1_ST_REASON = 1, PD1_ST_T = 2, PD1_ST_K = 3, PD1_ST_WORDS = 4 };
enum : uint32_t { PD1_GO = 1, PD1_SKIP = 2 };
enum : uint32_t { PD1_R_NONE = 0, PD1_R_STATE = 1, PD1_R_VCAP = 2, PD1_R_FAIL = 3, PD1_R_CAP = 4, PD1_R_DCAP = 5,
                  PD1_R_LARGE = 6 };
enum { GP1_ST_STATE = 0, GP1_ST_RUN = 1, GP1_ST_SKIPPED = 2, GP1_ST_G = 3, GP1_ST_P = 4, GP1_ST_N = 5, GP1_ST_WORDS = 6 };
enum : uint32_t { GP1_GROUPED = 1, GP1_SKIPPED = 2 };
hipError_t launch_pd_gate(const uint32_t *status_in, const uint64_t *head, const uint32_t *dest_offsets, uint32_t n_dests,
                          const uint32_t *fail, uint64_t vcap, uint64_t cap, uint64_t dcap, uint64_t tmax, uint64_t nmax,
                          uint64_t *out_head, uint32_t *gate, uint32_t *status, hipStream_t s);
hipError_t launch_group_picks_one(const uint32_t *gate, const uint64_t *head, const uint32_t *in_topic,
                                  const uint32_t *in_value, const uint32_t *in_sub, const uint32_t *dest_offsets,
                                  uint32_t n_dests, const uint32_t *e_topic, const uint32_t *e_value, const uint32_t *member,
                                  const uint32_t *sub_of, uint64_t sub_of_len, uint64_t cap, uint64_t dcap,
                                  uint32_t *out_member, uint32_t *out_dtopic, uint32_t *out_dvalue, uint32_t *out_dsub,
                                  uint64_t *out_ghead, uint32_t *out_gsub, uint32_t *out_goff, uint64_t gcap,
                                  uint32_t *status, hipStream_t s);
// delta upload: run i copies runs[i].n u32 words from data + runs[i].src to
// word (dst & PATCH_OFF) of table (dst >> 48), whose device address on the
// replica being patched is bases.b[table] (the same runs patch every replica)
constexpr int N_TABLES = 9;   // vocab, wpool, nodes, ctab, vals, exact, xfp, wseq, wbits
constexpr uint64_t PATCH_OFF = (1ull << 48) - 1;
struct PatchRun { uint64_t dst; uint32_t src, n; };
struct PatchBases { uint64_t b[N_TABLES]; };
hipError_t launch_patch(const PatchRun *d_runs, const uint32_t *d_data, uint64_t n_runs, PatchBases bases,
                        hipStream_t s);
// matches_filter/3 over the term-ordered word-list keys (pass 1: hit == null, per-query counts; pass 2: values)
hipError_t launch_matches_filter(uint64_t n, const uint32_t *qoff, const uint32_t *qr, const uint32_t *qbase,
                                 const uint32_t *pool, const uint64_t *koff, const uint32_t *kval, uint64_t K,
                                 uint32_t *cnt, const uint64_t *hit, uint32_t *out, uint64_t cap, uint8_t *err,
                                 hipStream_t s);

}  // namespace tmx
