/*
 * tmatch.h -- C ABI of the MI355X topic-match engine (libtmatch.so).
 *
 * Drop-in boundary for EMQX's publish-routing match path.  Plain C types only:
 * pointers, sizes, status codes; no exceptions cross this boundary.  What each
 * entry point replaces in the reference (paths relative to the reference root):
 *
 *   tm_create / tm_create_replicas / tm_destroy
 *       emqx_topic_index:new/0,1          apps/emqx/src/emqx_topic_index.erl:40-48
 *       (replicas: the node-wide replicated route table, emqx_router.erl:133-162)
 *       (the ETS ordered_set stays the source of truth on the Erlang side; this
 *        handle is its HBM mirror -- SURVEY.md 8b "Ownership")
 *   tm_apply_deltas
 *       emqx_topic_index:insert/4, delete/3 apps/emqx/src/emqx_topic_index.erl:53-62
 *       via emqx_trie_search:make_key/2     apps/emqx/src/emqx_trie_search.erl:115-128
 *       and the router's batched writes     apps/emqx/src/emqx_router.erl:255-273,483-509
 *   tm_match_batch / tm_match_batch_dev
 *       emqx_topic_index:matches/3          apps/emqx/src/emqx_topic_index.erl:76-78
 *       = emqx_trie_search:matches/3        apps/emqx/src/emqx_trie_search.erl:182-226,381-389
 *       called per publish by emqx_router:match_routes/1 (emqx_router.erl:205-212,511-516)
 *   tm_first_batch
 *       emqx_topic_index:match/2            apps/emqx/src/emqx_topic_index.erl:70-72
 *       (first key in traversal order; emqx_trie_search.erl:171-178,350-356)
 *   tm_apply_deltas_ex, tm_read_begin / tm_read_end / tm_epoch
 *       safe reuse of u32 values under lock-free readers (see "Reader epochs";
 *       emqx_topic_index.erl:41-48 is the read_concurrency contract kept)
 *   tm_stats
 *       emqx_router:stats/1 n_routes part    apps/emqx/src/emqx_router.erl:632-635
 *   tm_merge_shards
 *       no reference counterpart: the reference holds every route on every
 *       node (mria-replicated emqx_route_filters, emqx_router.erl:105-108);
 *       filter sets beyond one GPU are split into shards and the
 *       shards' hit lists, allgathered over RCCL, are merged by this call so
 *       the result equals emqx_topic_index:matches/3 over the whole set
 *
 * Keys.  An index entry is the pair (filter, value).  `value` is a caller-chosen
 * u32 (the NIF interns the Erlang {ID} term, or the whole key, to a u32).
 * Key form follows make_key/2: a binary filter with a '+'/'#' level is a word
 * list; a binary without one is a binary key; TM_KEY_WORDS forces the
 * word-list form (make_key(Words, ID) with a list); TM_KEY_EMPTY_LIST is the
 * word list [] (which has no byte form).  TM_KEY_WORDS | TM_KEY_ESCAPED is
 * a word list whose binary words may hold any bytes: words are separated by
 * '/', and inside a word "\/" stands for a '/' byte and "\\" for a '\';
 * a word written "\+" or "\#" is the binary word <<"+">> / <<"#">>, where
 * a bare "+" / "#" is the wildcard ('+' / '#' atoms).  A key with such a
 * word can never match a publish topic (a topic level is never "+" or "#",
 * never holds a '/'), but it is one of the table's keys for matches_filter/3
 * (tm_matches_filter), where it takes its place in Erlang term order.
 * Inserting an existing key and deleting a missing key are no-ops (ETS set
 * semantics, emqx_topic_index.erl:58-62).
 *
 * Output.  For each topic the matching values are written in TRAVERSAL order:
 * ascending Erlang term order of the keys {Filter, {Value}} -- word-list keys
 * (by word: '#' < '+' < binary words, shorter first), then binary keys, and
 * ascending value inside one filter.  This is exactly the order in which the
 * reference's walk visits them; its matches/3 list is the reverse
 * (match_add/2 prepends, emqx_trie_search.erl:353-354).
 * A topic with a level equal to "+" or "#" is badarg (emqx_trie_search.erl:374-375):
 * its err flag is 1 and it has no hits.
 * A topic of more than 65536 levels (longer than MQTT's 65535-byte maximum,
 * emqx_mqtt.hrl:44, so never seen from a client) is not matched: err flag 2,
 * no hits.  Err flag 4 marks a topic whose batch failed inside the device
 * (the bounded wait of a one-launch batch's look-back scan expired -- never
 * expected: a block waits only for blocks already running); its offsets and
 * values are undefined.  It is never a client error (the reference raises
 * badarg only for a '+'/'#' level): the host API (tm_match_batch*) runs such
 * a batch again once and returns TM_EDEVICE if it fails again, so its callers
 * never see err 4; a device-API caller (tm_match_batch_dev*, asynchronous)
 * finds the flags in d_out_err and submits the batch again.
 *
 * Forward progress (k_walk_small's look-back).  A block of a
 * one-launch batch waits only for blocks of its own launch (segment) that
 * come before it.  In dispatch order (TM_DEBUG_SMALL_TICKET 0), "before" is
 * blockIdx: the command processor hands a launch's workgroups to the 8 XCDs
 * round robin and each XCD starts its share in index order, so within ONE
 * launch the lowest unfinished block never waits for an unstarted one once
 * the blocks below it have left their XCD -- but the XCDs start their shares
 * independently, and with several look-back launches in flight (concurrent
 * callers, the combiner's leaders) every slot of one XCD can be held by
 * waiting blocks of one launch while the predecessor they wait for sits
 * unstarted behind another launch's waiting blocks on another XCD.  So
 * dispatch order alone does not guarantee progress on gfx950; the bounded
 * wait turns such a stall into err 4 (a rerun, then TM_EDEVICE), never a
 * wrong result.  With a start-order ticket (TM_DEBUG_SMALL_TICKET 1, the
 * default since round 6: measured free) a block
 * takes its index from an atomic counter when it starts, so every block it
 * waits for has started and runs to its publication without waiting for a
 * later one: progress by construction.
 */
#ifndef TMATCH_H
#define TMATCH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tm_index tm_index;

enum {
    TM_OK = 0,
    TM_EINVAL = -1,   /* bad argument (null pointer, bad op code)            */
    TM_ENOMEM = -2,   /* host or device allocation failed                    */
    TM_EDEVICE = -3,  /* HIP runtime error                                   */
    TM_ECAP = -4      /* output capacity too small: offsets are valid, ids   */
                      /* were truncated to `cap`; retry with cap >= total    */
};

enum { TM_OP_DELETE = 0, TM_OP_INSERT = 1 };
enum { TM_KEY_BINARY = 0, TM_KEY_WORDS = 1, TM_KEY_EMPTY_LIST = 2, TM_KEY_ESCAPED = 4 };

typedef struct {
    int32_t device;          /* HIP device ordinal; -1 = current device        */
    uint32_t copies;         /* copies of the tables per device (0 = 1; <= 4):
                                with 2 or more a batch after a delta runs on a
                                copy no batch is reading, which takes the delta
                                at once, instead of waiting for the batches in
                                flight on a single copy (churn, C5); without
                                deltas every batch reads the first copy       */
    uint64_t hint_keys;      /* expected number of keys (sizes tables up front) */
} tm_options;

typedef struct {
    uint64_t n_keys;         /* live keys (word-list + binary + never-matching) */
    uint64_t n_wild_keys;    /* word-list keys (trie terminals)                 */
    uint64_t n_exact_keys;   /* binary keys                                     */
    uint64_t n_dead_keys;    /* keys that can never match ('#' not last, [])     */
    uint64_t n_nodes, n_edges, n_words;
    uint64_t device_bytes;   /* HBM held by the mirror                          */
    uint64_t uploads;        /* full + patch uploads performed                   */
    uint64_t patch_bytes;    /* bytes moved by incremental patches              */
} tm_stats_t;

/* Create an empty index on a device.  opts may be NULL. */
int tm_create(const tm_options *opts, tm_index **out);
int tm_destroy(tm_index *h);

/* One host image, n device replicas (1 <= n <= 8; a device may repeat):
 * the topic-sharded mode of SURVEY.md 8e in one process, as one EMQX node
 * (one BEAM VM) drives all its GPUs.  The reference keeps one replicated route
 * table per node (emqx_router.erl:133-162); here the host key set, its
 * compiler and tm_apply_deltas run once, and every patch's staged runs are
 * copied to every replica (one pinned buffer, one H2D copy + one patch kernel
 * per device), lazily: a replica takes the patches logged since its last batch
 * when a batch is about to run there.  Each device entry holds opts->copies
 * copies (replica r is copy r % copies of device entry r / copies).  Host-API
 * batches go to the device entry with the fewest batches in flight (round
 * robin among equals); device-API calls use the entry of the calling thread's
 * current HIP device (the first one there); within an entry a batch reads its
 * first up-to-date copy, else a copy no batch is reading, else the least
 * recently used one.  opts->device is ignored; matches_filter runs on replica
 * 0.  tm_stats().device_bytes is per replica. */
int tm_create_replicas(const tm_options *opts, const int32_t *devices, uint32_t n, tm_index **out);

/* Batches (host and device API) replica r has served so far, and its device. */
int tm_replica_stats(tm_index *h, uint32_t r, uint64_t *batches, int32_t *device);

/* Apply n deltas in order (a later op on the same key wins).  Host buffers:
 * filter i is filter_bytes[filter_offsets[i] .. filter_offsets[i+1]).
 * key_flags may be NULL (all TM_KEY_BINARY).  Device upload is deferred to the
 * next match / tm_sync on the stream given there (patches are applied in
 * stream order, so a batch sees exactly the deltas applied before it). */
int tm_apply_deltas(tm_index *h, uint64_t n, const uint8_t *ops, const uint8_t *filter_bytes,
                    const uint64_t *filter_offsets, const uint32_t *values, const uint8_t *key_flags);

/* tm_apply_deltas, also returning the delta epoch the batch made current
 * (*out_epoch, may be NULL): every call with n > 0 advances the index's epoch
 * by one (see "Reader epochs" below). */
int tm_apply_deltas_ex(tm_index *h, uint64_t n, const uint8_t *ops, const uint8_t *filter_bytes,
                       const uint64_t *filter_offsets, const uint32_t *values, const uint8_t *key_flags,
                       uint64_t *out_epoch);

/* tm_apply_deltas_ex for a writer that must not slow the readers: the route
 * mirror's group commit (src/emqx_router_gpu.erl, the read-your-writes hook
 * of emqx_router.erl:483-509 under the broker pool's concurrent route writes,
 * emqx_broker.erl:778-808).  The deltas are applied to the host image, the
 * resulting patch is shipped to a copy of the tables (tm_options.copies) that
 * no batch is reading, and only then published: it returns once every batch
 * queued afterwards reads a copy holding these deltas (as tm_apply_deltas
 * does), but no batch waits on the GPU for the patch -- with tm_apply_deltas
 * every batch after a delta first waits for the batches still reading the
 * copy it patches.  While every copy has readers, tm_commit waits for one to
 * drain (bounded; past the bound, or with copies = 1 -- then whether the copy
 * has readers or not -- it publishes as tm_apply_deltas does).  It never
 * waits when the deltas changed more than logged words: a table shipped
 * whole (growth, a rehash, more than half of it dirty) or a change of what a
 * launch is told about the tables (their addresses and sizes, the trie's
 * depth, the lengths binary keys have) reaches every copy at once, so such a
 * commit publishes at once too, and every batch queued from then on first
 * brings its copy up.  Batches do not collect these deltas before
 * tm_commit publishes them (they were queued before it returned); a
 * tm_apply_deltas running meanwhile is published with them. */
int tm_commit(tm_index *h, uint64_t n, const uint8_t *ops, const uint8_t *filter_bytes, const uint64_t *filter_offsets,
              const uint32_t *values, const uint8_t *key_flags, uint64_t *out_epoch);

/* Reader epochs: when may a caller hand a value freed by a delete to a new key?
 * The reference's readers walk a read_concurrency ETS table and decode keys
 * from it lock-free (emqx_topic_index.erl:41-48): a concurrent delete can hide
 * a key, but a reader never sees a key that does not match.  Here a reader gets
 * u32 values back and turns them into keys afterwards, so a value must not be
 * reused while a reader that may still return it is running:
 *   tm_read_begin   registers a reader at the current epoch (before it queues
 *                   its batches); *ticket identifies it;
 *   tm_read_end     unregisters it (after it has decoded its results);
 *   tm_epoch        *current = the index's epoch, *safe = the smallest epoch
 *                   of a registered reader (= *current when there is none).
 * A value freed by a delete that tm_apply_deltas_ex reported as epoch E may be
 * reused once *safe >= E: every reader still running began after the delete,
 * and its batches cannot see the old key.  No reference counterpart (ETS
 * keys are their own identity).  Thread safe; never blocks on the GPU. */
int tm_read_begin(tm_index *h, uint64_t *ticket);
int tm_read_end(tm_index *h, uint64_t ticket);
int tm_epoch(tm_index *h, uint64_t *current, uint64_t *safe);

/* Upload pending patches on `stream` (hipStream_t; NULL = the default stream). */
int tm_sync(tm_index *h, void *stream);

/* Host buffers in, host buffers out (pinned staging inside).  Blocks until the
 * hit lists are in host memory.  out_hit_offsets has n+1 entries;
 * out_err has n entries (may be NULL).
 * Thread safety: any number of threads may call tm_match_batch,
 * tm_first_batch and tm_apply_deltas on one index at once (the reference's
 * readers run concurrently on a read_concurrency ETS table,
 * emqx_topic_index.erl:41-48).  Each host-API batch runs on its own stream
 * with its own scratch (up to 16 in flight; more callers wait for one), and
 * the index lock is held only while pending deltas are shipped and the
 * kernels are queued, never while waiting for the GPU.  A batch sees every
 * delta applied before it was queued. */
int tm_match_batch(tm_index *h, uint64_t n, const uint8_t *topic_bytes, const uint64_t *topic_offsets,
                   uint64_t *out_hit_offsets, uint32_t *out_values, uint64_t cap, uint8_t *out_err);

/* Output order of a topic's hit list:
 *   TM_ORDER_TRAVERSAL  the reference's traversal order (see "Output" above)
 *   TM_ORDER_SORTED     ascending u32
 *   TM_ORDER_UNIQUE     ascending u32 without repeats -- matches/3 with
 *                       [unique] (emqx_trie_search.erl:201-211) when the NIF
 *                       interns IDs (not whole keys) to u32: the distinct
 *                       values come first in the topic's segment, the rest of
 *                       the segment is 0xFFFFFFFF, and out_unique[i] (n
 *                       entries, may be NULL) is topic i's distinct count.
 * Offsets are the same in every order. */
enum { TM_ORDER_TRAVERSAL = 0, TM_ORDER_SORTED = 1, TM_ORDER_UNIQUE = 2 };

int tm_match_batch_ex(tm_index *h, uint64_t n, const uint8_t *topic_bytes, const uint64_t *topic_offsets,
                      uint64_t *out_hit_offsets, uint32_t *out_values, uint64_t cap, uint8_t *out_err,
                      uint32_t order, uint32_t *out_unique);

/* tm_match_batch_ex with 32-bit offsets: topic_offsets[n+1] and
 * out_hit_offsets[n+1] are u32 (a batch's topic bytes and its values must each
 * stay below 2^32 -- a NIF micro-batch always does).  An in-place batch of up
 * to 65536 topics (see tm_host_alloc) in TM_ORDER_TRAVERSAL then moves half
 * the offset bytes over PCIe in each direction; any other batch is widened to
 * tm_match_batch_ex on the host.  cap is clamped to 2^32 - 1; TM_EINVAL if the
 * values exceed that.  (No reference counterpart: the NIF's own buffers.) */
int tm_match_batch32_ex(tm_index *h, uint64_t n, const uint8_t *topic_bytes, const uint32_t *topic_offsets,
                        uint32_t *out_hit_offsets, uint32_t *out_values, uint64_t cap, uint8_t *out_err,
                        uint32_t order, uint32_t *out_unique);

/* tm_match_batch32_ex in TM_ORDER_TRAVERSAL with the hit lists as per-topic
 * (first position, count) pairs instead of a CSR: out_pairs[2 i] is topic i's
 * first value in out_values, out_pairs[2 i + 1] its count, out_pairs[2 n] the
 * values' total (TM_ECAP when it exceeds cap: the pairs are valid, values past
 * cap dropped).  A topic's values are contiguous and in traversal order, as
 * in the CSR; the topics' spans are disjoint but NOT in topic order.  What
 * the NIF binds (c_src/tmatch_nif_core.c tmn_row): an in-place batch (every
 * buffer from tm_host_alloc / TM_ALLOC_VRAM) of up to 65536 topics runs in
 * one launch whose blocks each reserve their values' span with one atomic
 * and never wait for another block (no cross-block scan: a finished block
 * frees its slot at once for concurrent callers' launches, and forward
 * progress needs no argument); any other batch takes tm_match_batch32_ex and
 * is converted.  out_err is required (n entries).  (No reference counterpart:
 * the NIF builds each topic's list from its span.) */
int tm_match_batch32_pairs(tm_index *h, uint64_t n, const uint8_t *topic_bytes, const uint32_t *topic_offsets,
                           uint32_t *out_pairs, uint32_t *out_values, uint64_t cap, uint8_t *out_err);

/* tm_match_batch_dev with 32-bit offsets (traversal order): a batch of up to
 * 65536 topics reads and writes them as they are; a larger one is widened
 * into the stream's scratch, matched and narrowed on the device (two small
 * copy kernels).  For host-fed pipelines: 4 B per topic less each way. */
int tm_match_batch32_dev(tm_index *h, uint64_t n, const uint8_t *d_topic_bytes, const uint32_t *d_topic_offsets,
                         uint32_t *d_out_hit_offsets, uint32_t *d_out_values, uint64_t cap, uint8_t *d_out_err,
                         void *stream);

/* Pinned host buffers, mapped into the index's device.  A NIF keeps its
 * per-scheduler batch buffers here: when every buffer given to tm_match_batch
 * (topic bytes -- 16-byte aligned --, offsets, hit offsets, values and err if
 * not NULL) lies in tm_host_alloc memory of the same index and n <= 65536, the
 * kernels read the topics and write the hit lists in place: no staging copy
 * in, no copy out.  The same holds for tm_first_batch (out_value, out_found).
 * Other batches take the staged path; results are the same.
 * tm_host_free waits for the index's batches to finish first. */
int tm_host_alloc(tm_index *h, uint64_t bytes, void **out);
int tm_host_free(tm_index *h, void *p);

/* tm_host_alloc with flags.  TM_ALLOC_VRAM: device memory of the index's GPU
 * (fine-grained HBM) mapped into the host's address space through the PCIe
 * BAR, for a batch's INPUTS (topic bytes, offsets): the host writes it with
 * ordinary stores (write-combined: ~37 GB/s for a 4k-topic batch's 140 KB,
 * tools/study/bar_probe.hip), and an in-place batch's kernel then reads HBM --
 * no PCIe read on its critical path.  Host READS of it are uncached PCIe reads
 * (~0.6 us each): write it, never read it back.  Outputs stay in tm_host_alloc
 * memory.  Only on an index with one device (TM_EINVAL for replicas); freed by
 * tm_host_free.  flags 0 = tm_host_alloc.  (No reference counterpart: the
 * NIF's own buffers.) */
#define TM_ALLOC_VRAM 1u
int tm_host_alloc_ex(tm_index *h, uint64_t bytes, uint32_t flags, void **out);

/* Device-resident batch: every pointer is device memory; asynchronous on
 * `stream` (hipStream_t; NULL = HIP's default stream, which PyTorch's default
 * stream handle 0 also names).  d_out_hit_offsets has
 * n+1 entries and d_out_hit_offsets[n] is the total; values beyond `cap` are
 * dropped (the caller compares the total with cap after synchronising).
 * The library keeps batch scratch for the 16 most recently used streams (an
 * older stream's is released after its batches finish). */
int tm_match_batch_dev(tm_index *h, uint64_t n, const uint8_t *d_topic_bytes, const uint64_t *d_topic_offsets,
                       uint64_t *d_out_hit_offsets, uint32_t *d_out_values, uint64_t cap,
                       uint8_t *d_out_err, void *stream);

int tm_match_batch_dev_ex(tm_index *h, uint64_t n, const uint8_t *d_topic_bytes, const uint64_t *d_topic_offsets,
                          uint64_t *d_out_hit_offsets, uint32_t *d_out_values, uint64_t cap,
                          uint8_t *d_out_err, uint32_t order, uint32_t *d_out_unique, void *stream);

/* tm_match_batch_dev (traversal order) with the hit lists as per-topic (first
 * position, count) pairs: d_out_pairs[2 i] / [2 i + 1] (u32; the array 8-byte
 * aligned, 2 n + 2 entries), d_out_pairs[2 n] the values' total and
 * d_out_pairs[2 n + 1] the extent -- the end of the highest position used
 * (both saturated at 2^32 - 1; cap is clamped to 2^32 - 1).  Each topic's
 * values are contiguous and in traversal order; the topics' spans are disjoint,
 * NOT in topic order, and may leave gaps: each walk block reserves its span
 * with one atomic in one of up to 64 regions of the output (together 7/8 of
 * cap; one region per 8192 topics) or, when its region is full, in the pool
 * above them, so no counter is hot.  extent > cap means values were dropped (a
 * topic whose first position + count exceeds cap lost those values: submit
 * the batch again with a larger cap).  With one region (batches below 16k
 * topics) none are when cap >= total + 64 x the most hits of one topic (a
 * region's last reservation that did not fit wastes its tail); a larger
 * batch needs cap >= total + 4096 x the most hits of one topic and every
 * region to receive at least 7/8 of an even share of the values (its ~128+
 * walk blocks' topics are interleaved with the other regions' 64 apart, so a
 * batch whose hits are not laid out in a period of 64 topics meets it); for
 * any layout, cap >= 8 x (total + 64 x the most hits of one topic) is enough
 * (the pool alone then holds every value).
 * Two launches per batch: the walk writes its own topics' values (no
 * cross-block scan, no range lists, no emit kernel), then one small kernel
 * finishes the topics deeper than the walk's level store and those with more
 * than 8 value runs.  For a consumer that builds one list per topic (the NIF, a
 * fan-out stage): the same lists as tm_match_batch_dev, fewer passes over HBM.
 * (No reference counterpart: emqx_topic_index:matches/3 per topic,
 * emqx_topic_index.erl:54-57.) */
int tm_match_batch_dev_pairs(tm_index *h, uint64_t n, const uint8_t *d_topic_bytes, const uint64_t *d_topic_offsets,
                             uint32_t *d_out_pairs, uint32_t *d_out_values, uint64_t cap, uint8_t *d_out_err,
                             void *stream);

/* Sort each segment of a device CSR (n segments, d_hit_offsets[n+1]) in
 * place in TM_ORDER_SORTED / TM_ORDER_UNIQUE order (d_out_unique as above),
 * asynchronously on `stream`: e.g. the merged lists of tm_merge_shards, which
 * then equal one index's sorted lists exactly.  Segments past `cap` values are
 * left alone. */
int tm_sort_segments(tm_index *h, uint64_t n, const uint64_t *d_hit_offsets, uint32_t *d_values, uint64_t cap,
                     uint32_t order, uint32_t *d_out_unique, void *stream);

/* Route fan-out: hit lists bucketed by destination.
 * emqx_broker:do_publish/1 is route(aggre(match_routes(Topic)), Delivery)
 * (emqx_broker.erl:293-298): each hit is a route {To, Dest}, and do_route2/2
 * (emqx_broker.erl:401-406) dispatches it locally, forwards it to
 * get_dest_node(Dest) (emqx_router.erl:580-585) with forward/4
 * (emqx_broker.erl:429), or hands it to a shared group -- once per hit.  A
 * batched broker forwards once per destination per micro-batch, so it needs
 * the batch's (topic, value) pairs grouped by the destination of the value.
 *
 * tm_set_dests: the index's value -> destination table (the caller's dense
 * ids, e.g. one per node, per shared group and per external destination;
 * get_dest_node/1 on the interned route).  A value never set is unrouted.
 * Thread safe with every other call; a fan-out queued after it returns sees the
 * new table (only the entries changed since a device's last fan-out are
 * uploaded, in stream order before it), one already queued may see either
 * state.  Set a value's destination before inserting its key; the reader
 * epochs above already keep a freed value from being reused early.  The host
 * table has one u32 per value up to the largest one set.
 *
 * tm_fanout_dev: device buffers, asynchronous on `stream`.  Input: any device
 * CSR -- d_hit_offsets[n + 1] and d_values as tm_match_batch_dev or
 * tm_merge_shards write them (tm_match_batch_dev_pairs' and
 * tm_match_batch32_pairs' pairs go to tm_fanout_dev_pairs below: their spans
 * are not in topic order) -- and d_dest_of[dest_len] (NULL: the index's own
 * table, dest_len ignored).  The entry at position p < min(d_hit_offsets[n],
 * cap) has topic t (the segment holding p), value v = d_values[p] and bucket
 * b = d_dest_of[v] if v < dest_len and d_dest_of[v] < n_dests, else b =
 * n_dests: the unrouted bucket, so nothing is dropped.  Output:
 * d_dest_offsets[n_dests + 2], the exclusive scan of the bucket sizes with
 * the total last, and d_out_topic / d_out_value (u32): bucket b's entries at
 * [d_dest_offsets[b], d_dest_offsets[b + 1]) in ascending input position
 * (ascending topic, traversal order inside a topic) -- numpy.argsort(bucket,
 * kind="stable") applied to (topic, value).  Entries at positions >= cap
 * (clamped to 2^32 - 1) are neither counted nor written, and nothing past
 * min(total, cap) is written in either array; the inputs are not modified.
 * One pass over the entries for n_dests + 1 <= 256, two otherwise (then the
 * stream's scratch holds 12 bytes x cap: TM_ENOMEM if that cannot be had).
 * Scratch is kept per stream with the batch scratch (tm_stream_release).
 *
 * tm_route_batch: host buffers in and out, the product path -- the batch is
 * matched into device scratch (CSR, traversal order), fanned out with the
 * index's table, and the three arrays are copied back.  out_dest_offsets has
 * n_dests + 2 entries, out_topic / out_values `cap`; out_err as for
 * tm_match_batch (may be NULL).  Concurrency, lanes and the device-failure
 * retry are tm_match_batch's.  TM_ECAP when the total exceeds cap: the first
 * cap entries are written and out_dest_offsets still holds the full bucket
 * sizes, so the caller sizes its retry from out_dest_offsets[n_dests + 1].
 *
 * tm_fanout_dev_pairs (ABI minor 12): tm_fanout_dev for a batch given as
 * per-topic (first position, count) pairs, as tm_match_batch_dev_pairs and
 * tm_match_batch32_pairs write them; everything else (buffers, stream, lanes,
 * scratch, thread safety, d_dest_of == NULL) as tm_fanout_dev.  d_pairs is u32
 * and 8-byte aligned; for topic t, pos_t = d_pairs[2 t] and cnt_t =
 * d_pairs[2 t + 1].  Only entries [0, 2 n) are read (the producers' totals and
 * extent after them are neither trusted nor needed).  cap (clamped to
 * 2^32 - 1) is the size of d_values and of both output arrays.  Definition:
 *   eff_t = 0 if pos_t >= cap, else min(cnt_t, cap - pos_t);
 *   the virtual CSR is hit'[t] = the sum of eff_u for u < t (64-bit sums: no
 *   input wraps) and vals'[hit'[t] + j] = d_values[pos_t + j];
 *   the outputs are exactly what tm_fanout_dev(n, hit', vals', cap, ...)
 *   writes: E = min(hit'[n], cap) entries, bucket b at [d_dest_offsets[b],
 *   d_dest_offsets[b + 1]) in ascending topic order, traversal order inside a
 *   topic, d_dest_offsets[n_dests + 1] = E, bucket n_dests the values without
 *   a destination; nothing at or past E is written in either output array,
 *   nothing past d_dest_offsets[n_dests + 1].
 * So no d_values word at or past cap is ever read; overlapping or repeated
 * spans are defined (read twice, dropped once the virtual position reaches
 * cap) and can never make the kernels write outside the outputs; the inputs
 * are not modified.  Three launches more than tm_fanout_dev (two scan the
 * effective counts, no block waiting for another; one resolves the entries),
 * and the stream's scratch holds 8 bytes x n and 12 bytes x cap for every
 * n_dests, 16 x cap for two passes (TM_ENOMEM if that cannot be had).
 *
 * tm_route_batch32 (ABI minor 13): tm_route_batch with 32-bit offsets in and
 * out, for a NIF's micro-batches.  The outputs are exactly those
 * tm_route_batch writes for the same index state, topics, n_dests and cap:
 * out_dest_offsets (u32, n_dests + 2 entries) holds the full bucket sizes even
 * under TM_ECAP, the first min(total, cap) entries of out_topic / out_values
 * are written and nothing at or past that in either array; TM_ECAP when
 * total > cap.  out_err is required.  Thread safety, lanes, read-your-writes
 * and the device-failure retry are tm_route_batch's.
 * In place -- no staging copy in, no copy out, one synchronisation -- when
 * n <= 8192 and n_dests <= 255 (the one-launch fan-out kernel's bounds), the
 * topic bytes are 16-byte aligned, every buffer (the inputs, which may be
 * TM_ALLOC_VRAM, the three outputs and out_err) lies in this index's
 * tm_host_alloc memory, and the index allows the one-launch walk (as
 * tm_match_batch32_pairs).  Then the batch is matched by the one-launch pairs
 * kernel, on the call's own lane, into the lane's scratch (8 bytes x n of pairs
 * and the values: at least 65536 and 4 n words, grown and the batch run again
 * when the total exceeds them; the flags go straight to out_err), and ONE
 * launch of one workgroup fans it out into the caller's buffers: no block
 * waits for another.  A batch with more than 16384 entries is finished on the
 * same lane by tm_fanout_dev_pairs' kernels on the pairs already matched (no
 * second walk; 12 bytes x total of scratch more) and copied out.  Every other
 * batch is widened on the host, run by tm_route_batch, and narrowed.
 * TM_DEBUG_ROUTE_ONE / TM_DEBUG_ROUTE_GRID (tm_debug_get) count the calls the
 * one-launch kernel completed / the grid kernels or the staged path finished.
 *
 * TM_EINVAL (before any device work): a null handle, a null required pointer,
 * n_dests == 0 or n_dests > 65536, n >= 2^32 - 1, d_pairs not 8-byte
 * aligned; tm_route_batch and tm_route_batch32 also when the batch's total
 * exceeds 2^32 - 1 (found on the device). */
int tm_set_dests(tm_index *h, uint64_t n, const uint32_t *values, const uint32_t *dests);
int tm_fanout_dev(tm_index *h, uint64_t n, const uint64_t *d_hit_offsets, const uint32_t *d_values, uint64_t cap,
                  const uint32_t *d_dest_of, uint64_t dest_len, uint32_t n_dests,
                  uint64_t *d_dest_offsets, uint32_t *d_out_topic, uint32_t *d_out_value, void *stream);
int tm_fanout_dev_pairs(tm_index *h, uint64_t n, const uint32_t *d_pairs, const uint32_t *d_values, uint64_t cap,
                        const uint32_t *d_dest_of, uint64_t dest_len, uint32_t n_dests,
                        uint64_t *d_dest_offsets, uint32_t *d_out_topic, uint32_t *d_out_value, void *stream);
int tm_route_batch(tm_index *h, uint64_t n, const uint8_t *topic_bytes, const uint64_t *topic_offsets,
                   uint32_t n_dests, uint64_t *out_dest_offsets, uint32_t *out_topic, uint32_t *out_values,
                   uint64_t cap, uint8_t *out_err);
int tm_route_batch32(tm_index *h, uint64_t n, const uint8_t *topic_bytes, const uint32_t *topic_offsets,
                     uint32_t n_dests, uint32_t *out_dest_offsets, uint32_t *out_topic, uint32_t *out_values,
                     uint64_t cap, uint8_t *out_err);

/* aggre/1 on the device (ABI minor 14): one entry per (To, destination).
 * emqx_broker:aggre/1 (emqx_broker.erl:408-424), the middle call of
 * do_publish/1, reduces {To, {Group, Node}} to {To, Group} and lists:usort's
 * the list: a shared group with members on k nodes -- k routes of one filter
 * -- gets a message once.  The calls above return match_routes' hits bucketed
 * by destination, the k copies included.  A topic's keys come in ascending
 * term order of their filters, the keys of one filter contiguous ("Output"),
 * and the fan-out is a stable partition; so inside one destination bucket the
 * entries of one topic that share a filter are adjacent, and the usort is
 * "drop an entry whose predecessor in the same bucket has the same topic and
 * the same filter".  Node routes are never touched ({Filter, Dest} keys are
 * unique), so no group flag is needed.
 *
 * tm_set_route_filters: the index's value -> To table, the twin of
 * tm_set_dests.  filter_ids[i] is the caller's id of the topic filter of the
 * route values[i] names: equal filters have equal ids, different live filters
 * different ids.  Ids are only compared, never index anything, and need not be
 * dense.  0xFFFFFFFF (also: never set) is "no filter known": such an entry
 * equals nothing and is never dropped.  Thread safe with every other call; an
 * aggre queued after it returns sees the new table (only the entries changed
 * since a device's last use are uploaded, in stream order before it), one
 * already queued may see either state.  Set a value's filter before inserting
 * its key.  The host table has one u32 per value up to the largest one set.
 *
 * tm_aggre_dev: device buffers, asynchronous on `stream`.  The input is what
 * tm_fanout_dev / tm_fanout_dev_pairs write: d_dest_offsets[n_dests + 2],
 * d_topic and d_value; E = min(d_dest_offsets[n_dests + 1], cap), cap clamped
 * to 2^32 - 1.  f(v) = d_filter_of[v] if v < filter_len, else 0xFFFFFFFF
 * (d_filter_of == NULL: the index's own table, filter_len ignored).  Entry
 * q < E is DROPPED iff q is not the first position of its bucket, q is not in
 * the unrouted bucket n_dests (which mixes classes the device cannot tell
 * apart and is copied whole), d_topic[q] == d_topic[q - 1] and
 * f(d_value[q]) == f(d_value[q - 1]) != 0xFFFFFFFF.  A run of k equal entries
 * keeps its first.  The definition holds for any input (merged shards whose
 * filters are not contiguous included); for one index's traversal order it
 * equals aggre/1.  In numpy:
 *   keep = ones(E); same = (t[1:E]==t[:E-1]) & (f[1:E]==f[:E-1]) & (f[1:E]!=NONE)
 *   keep[1:] = ~same; keep[doff[b]] = 1 for every b with doff[b] < E
 *   keep[min(doff[n_dests], E):] = 1
 *   out = entries[keep]; out_doff[b] = keep[:min(doff[b], E)].sum()
 * Output: the kept entries in input order in d_out_topic / d_out_value,
 * d_out_dest_offsets[b] = the number kept before min(d_dest_offsets[b], E),
 * d_out_dest_offsets[n_dests + 1] = the kept total K.  Nothing at or past K is
 * written in either output array, the inputs are not modified, no input
 * position >= E is read.  The outputs MUST NOT overlap the inputs.  Five
 * launches over the fan-out's fixed grid, no block waiting for another; the
 * stream's scratch (kept with the fan-out's, tm_stream_release) holds 12
 * bytes per 64 entries of cap and 16 KiB (TM_ENOMEM if that cannot be had).
 * It is sized from cap, not from the total, which only the device knows when
 * the call is queued: pass the size of the buffers (what the fan-out was
 * given), never 2^32 - 1 for "no bound" -- that asks for about 800 MB a stream.
 * TM_EINVAL before any device work: a null handle, a null required pointer,
 * n_dests == 0 or n_dests > 65536.
 *
 * tm_route_batch_ex / tm_route_batch32_ex: tm_route_batch / tm_route_batch32
 * with trailing flags.  flags == 0 is the old call exactly; TM_ROUTE_AGGRE
 * returns the aggregated buckets (the index's own filter table);
 * any other bit is TM_EINVAL.  With TM_ROUTE_AGGRE out_dest_offsets holds the
 * aggregated bounds, [n_dests + 1] = K, and only the K kept entries are
 * written.  TM_ECAP when the total BEFORE aggregation exceeds cap (the
 * fan-out needs that room): out_dest_offsets then holds the un-aggregated
 * bucket sizes -- an upper bound to size the retry from --, the entries are
 * undefined.  Lanes, read-your-writes, the device-failure retry and the
 * out_err rules are unchanged.  tm_route_batch_ex: match, fan-out and aggre
 * all in the lane's scratch.  tm_route_batch32_ex in place, under exactly
 * tm_route_batch32's conditions: the one-launch fan-out writes the lane's
 * scratch and a second launch of one workgroup compacts it into the caller's
 * buffers -- still one synchronisation and no copy out; past 16384 entries
 * the grid kernels run on the lane and the result is copied out.
 * TM_DEBUG_ROUTE_ONE / TM_DEBUG_ROUTE_GRID count these calls too. */
#define TM_ROUTE_AGGRE 1u
int tm_set_route_filters(tm_index *h, uint64_t n, const uint32_t *values, const uint32_t *filter_ids);
int tm_aggre_dev(tm_index *h, uint32_t n_dests, const uint64_t *d_dest_offsets, const uint32_t *d_topic,
                 const uint32_t *d_value, uint64_t cap, const uint32_t *d_filter_of, uint64_t filter_len,
                 uint64_t *d_out_dest_offsets, uint32_t *d_out_topic, uint32_t *d_out_value, void *stream);
int tm_route_batch_ex(tm_index *h, uint64_t n, const uint8_t *topic_bytes, const uint64_t *topic_offsets,
                      uint32_t n_dests, uint64_t *out_dest_offsets, uint32_t *out_topic, uint32_t *out_values,
                      uint64_t cap, uint8_t *out_err, uint32_t flags);
int tm_route_batch32_ex(tm_index *h, uint64_t n, const uint8_t *topic_bytes, const uint32_t *topic_offsets,
                        uint32_t n_dests, uint32_t *out_dest_offsets, uint32_t *out_topic, uint32_t *out_values,
                        uint64_t cap, uint8_t *out_err, uint32_t flags);

/* Local dispatch on the device (ABI minor 16): route hits expanded to
 * subscribers.  For a route on the local node do_route2/2 calls
 * emqx_broker:dispatch/2, and do_dispatch2/2 (emqx_broker.erl:726-760) looks
 * (message, To) up in the ?SUBSCRIBER bag and sends {deliver, To, Msg} to every
 * pid, shard rows {shard, I} expanded where they stand.  The calls above end
 * with the local node's bucket of (message, route) entries; these turn it into
 * the deliveries (message, route, subscriber).
 *
 * tm_set_subscribers: the index's value -> local subscriber list table, the
 * twin of tm_set_dests / tm_set_route_filters (it replaces the ?SUBSCRIBER
 * lookups of do_dispatch2/2).  For each i < n the list of route value
 * values[i] becomes subs[list_offsets[i] .. list_offsets[i + 1]), in the order
 * given -- the order do_dispatch2/2 visits, shard rows flattened by the caller.
 * An empty range is "no subscribers"; a value never set has none; a value named
 * twice in one call takes its last list.  Subscriber ids are the caller's
 * opaque u32s (interned pids), every u32 is legal.  Thread safe with every
 * other call; a dispatch queued after it returns sees the new lists (only the
 * words changed since a device's last use are uploaded, the pool before the
 * spans, in stream order before the dispatch and after the dispatches of other
 * streams that may still read the old copy), one already queued sees the old
 * or the new list of a value, never a mixture and never another value's words.
 * Set a value's subscribers before inserting its key.  On the host: 8 bytes per
 * value up to the largest one set, and the lists in a pool of power-of-two
 * blocks (at most 2^32 - 1 words) that is rewritten tight when more of it is
 * garbage than lists (TM_DEBUG_SUB_COMPACTIONS counts that).  TM_EINVAL before
 * any work: a null handle, a null required buffer with n > 0, decreasing
 * offsets, a list of more than 2^32 - 1 ids.  TM_ENOMEM as tm_set_dests.
 *
 * tm_dispatch_dev: device buffers, asynchronous on `stream`.  The input is what
 * tm_fanout_dev* or tm_aggre_dev wrote; `bucket` in [0, n_dests] (the unrouted
 * bucket is allowed), its bounds are read on the device.  d_sub_span[2 v],
 * d_sub_span[2 v + 1] = the position and count of value v's list in d_sub_pool
 * (span_len values, pool_len words; d_sub_span == NULL: the index's own table,
 * the other three ignored; else it must be 8-byte aligned).  cap and out_cap
 * are clamped to 2^32 - 1.  In numpy:
 *   E = min(doff[n_dests+1], cap); q0 = min(doff[bucket], E); q1 = min(doff[bucket+1], E); M = q1 - q0
 *   t, v = topic[q0:q1], value[q0:q1]
 *   pos, cnt = span[2v], span[2v+1] where v < span_len, else 0, 0
 *   cnt = 0 where pos + cnt > pool_len     (64-bit sum: a span outside the pool is empty, never read)
 *   off = [0] + cumsum(cnt) as u64;  T = off[M]
 *   src = repeat(arange(M), cnt);  r = arange(T) - off[src]
 *   out_topic, out_value, out_sub = t[src], v[src], pool[pos[src] + r]    -- the first W = min(T, out_cap)
 *   head = [M, T];  d_out_offsets[0..M] = off  (when given)
 * Nothing at or past W is written in the three output arrays, nothing past
 * d_out_offsets[M] and nothing past head[1]; the inputs are not modified; no
 * input position >= E and no pool word >= pool_len is read.  T > out_cap: the
 * caller reruns with room for T; head is exact either way.  The outputs MUST
 * NOT overlap the inputs.  Four launches over the fan-out's fixed grid, no
 * block waiting for another; the expansion shares out the OUTPUT positions, so
 * a 10^5-subscriber list is written by many blocks.  The stream's scratch
 * (kept with the fan-out's, tm_stream_release) holds 4 bytes x cap, 8 bytes x
 * (cap + 1) more when d_out_offsets is NULL, and 32 KiB (TM_ENOMEM if that
 * cannot be had).  It is sized from cap, not from the bucket, which only the
 * device knows when the call is queued: pass the size of the buffers, never
 * 2^32 - 1 for "no bound" -- that asks for about 50 GB a stream.
 * TM_EINVAL before any device work: a null handle, a null required pointer,
 * n_dests == 0 or n_dests > 65536, bucket > n_dests, d_sub_span given without
 * d_sub_pool while pool_len > 0, d_sub_span not 8-byte aligned.
 *
 * tm_dispatch_batch: the host product path -- tm_route_batch_ex(.., flags)
 * (flags 0 or TM_ROUTE_AGGRE; the index's own tables) followed, on the same
 * lane and in the same run, by the dispatch of bucket local_dest over the
 * fan-out's arrays (the aggre pass's under TM_ROUTE_AGGRE) with the index's
 * own subscriber table.  The route outputs and their TM_ECAP rule are exactly
 * tm_route_batch_ex's; out_head = [M, T] and the first min(T, dcap)
 * deliveries (out_dtopic, out_dvalue, out_dsub) are copied out as well;
 * TM_ECAP also when T > dcap, out_head[1] sizes the retry.  The lane's
 * delivery scratch grows from the T fetched with the results and only the
 * dispatch kernels are queued again: no second walk.  TM_EINVAL for
 * local_dest >= n_dests, a null out_head, null delivery buffers with dcap > 0,
 * and whatever tm_route_batch_ex refuses.  Lanes, read-your-writes, the
 * device-failure retry and the out_err rules are unchanged.
 *
 * tm_dispatch_batch32 (ABI minor 17): tm_dispatch_batch with 32-bit offsets in
 * and out, for a NIF's micro-batches.  For the same index state, topics,
 * n_dests, local_dest, flags, cap and dcap every output array and the return
 * code are what tm_dispatch_batch writes and returns, out_dest_offsets narrowed
 * to u32 (n_dests + 2 entries); out_head stays u64[2] = [M, T] (T is a 64-bit
 * sum) and must be 8-byte aligned.  Nothing is written at or past min(total,
 * cap) in out_topic / out_values, nothing at or past min(T, dcap) in the three
 * delivery arrays.  out_err is required.  TM_ECAP as tm_dispatch_batch: when
 * total > cap (the offsets hold the full sizes, before aggregation under
 * TM_ROUTE_AGGRE) and when T > dcap (out_head[1] sizes the retry).  TM_EINVAL:
 * whatever tm_route_batch32_ex refuses, local_dest >= n_dests, a null
 * out_head, null delivery buffers with dcap > 0, out_head not 8-byte aligned.
 * Lanes, read-your-writes and the device-failure retry are unchanged.
 * In place -- no staging copy in, no copy out, one synchronisation -- under
 * exactly tm_route_batch32's conditions, with out_head and the three delivery
 * arrays in this index's tm_host_alloc memory as well: the one-launch pairs
 * walk and the one-launch fan-out (and with TM_ROUTE_AGGRE the one-workgroup
 * aggre pass) write the lane's scratch, and ONE more launch of one workgroup
 * copies the route outputs, counts and scans the local bucket's subscriber
 * lists and expands them into the caller's buffers, which the device never
 * reads.  That workgroup expands at most 32768 deliveries (TM_DEBUG_DP1_MAX
 * lowers the bound); a local bucket with more, or a batch with more than 16384
 * entries, is finished on the same lane by tm_dispatch_dev's grid kernels on the
 * arrays already there (no second walk), which write the deliveries straight
 * into the caller's buffers.  Every other batch is widened on the host, run by
 * tm_dispatch_batch, and narrowed.  TM_DEBUG_DISPATCH_ONE /
 * TM_DEBUG_DISPATCH_GRID (tm_debug_get) count the calls the one-launch kernel
 * completed / the grid kernels or the staged path finished. */
int tm_set_subscribers(tm_index *h, uint64_t n, const uint32_t *values, const uint64_t *list_offsets,
                       const uint32_t *subs);
int tm_dispatch_dev(tm_index *h, uint32_t n_dests, const uint64_t *d_dest_offsets, uint32_t bucket,
                    const uint32_t *d_topic, const uint32_t *d_value, uint64_t cap,
                    const uint32_t *d_sub_span, uint64_t span_len, const uint32_t *d_sub_pool, uint64_t pool_len,
                    uint64_t *d_out_head, uint64_t *d_out_offsets,
                    uint32_t *d_out_topic, uint32_t *d_out_value, uint32_t *d_out_sub, uint64_t out_cap,
                    void *stream);
int tm_dispatch_batch(tm_index *h, uint64_t n, const uint8_t *topic_bytes, const uint64_t *topic_offsets,
                      uint32_t n_dests, uint32_t local_dest, uint32_t flags,
                      uint64_t *out_dest_offsets, uint32_t *out_topic, uint32_t *out_values, uint64_t cap,
                      uint64_t *out_head, uint32_t *out_dtopic, uint32_t *out_dvalue, uint32_t *out_dsub,
                      uint64_t dcap, uint8_t *out_err);
int tm_dispatch_batch32(tm_index *h, uint64_t n, const uint8_t *topic_bytes, const uint32_t *topic_offsets,
                        uint32_t n_dests, uint32_t local_dest, uint32_t flags,
                        uint32_t *out_dest_offsets, uint32_t *out_topic, uint32_t *out_values, uint64_t cap,
                        uint64_t *out_head, uint32_t *out_dtopic, uint32_t *out_dvalue, uint32_t *out_dsub,
                        uint64_t dcap, uint8_t *out_err);

/* Shared-subscription pick on the device (ABI minor 18): one member per
 * (message, group).  do_route2/2's third arm hands a {Group, _} destination to
 * emqx_shared_sub:dispatch/3 (apps/emqx/src/emqx_shared_sub.erl:146-163), which
 * looks the members of {Group, Topic} up and picks ONE of them by the group's
 * strategy (pick/6, do_pick/7, pick_subscriber/6: :335-406; the counter of
 * round_robin_per_group: :514-524).  aggre/1 has already reduced {To, {Group,
 * Node}} to {To, Group}, one entry per message, so the input is the aggregated
 * arrays tm_aggre_dev writes; the output is one member (or "no pick") per entry.
 * FailedSubs, {retry, _}, acks and the redispatch header stay on the host: a
 * failed send re-enters dispatch/4 there with the failed pid excluded.
 *
 * tm_set_share_slots: the index's value -> slot table, a twin of tm_set_dests
 * (same thread safety, upload discipline and errors).  A slot is the caller's
 * dense u32 id of a {Group, To} pair; the k routes {To, {Group, Node_i}} of one
 * pair share one slot.  TM_SHARE_NONE (0xFFFFFFFF): none; a value never set
 * has none.  Set a value's slot (and the slot's members) before inserting its
 * key.
 *
 * tm_set_share_members: for each i < n slot slots[i] takes the member list
 * members[list_offsets[i] .. list_offsets[i + 1]) -- interned pids in the order
 * of subscribers/2, which is what the exact parity of the two round robins and
 * the two hashes needs; under TM_SHARE_LOCAL (as the strategy, or as sticky's
 * initial pick) the caller puts the members on this node FIRST instead, since
 * the device picks among a prefix -- with n_local[i] (how many of the leading
 * members are local) and meta[i] = strategy | init_strategy << 8
 * (TM_SHARE_*; init_strategy is sticky's initial pick: TM_SHARE_RANDOM, _LOCAL,
 * _HASH_CLIENTID or _HASH_TOPIC, anything else picks as TM_SHARE_RANDOM).  A
 * slot named twice in one call takes its last list.  Member ids must be below
 * 0xFFFFFFFF, which is "no pick".  The call never touches a slot's state.
 * Thread safety and uploads as tm_set_subscribers (the lists live in a second
 * pool of the same kind; a pick takes the pool, the records and the slot table
 * in one hold of the lock); on the device one 16-byte record (pos, cnt,
 * n_local, meta) per slot up to the largest one set.  TM_EINVAL before any
 * work: a null handle, a null buffer with n > 0, decreasing offsets, a list of
 * more than 2^32 - 1 ids, slot 0xFFFFFFFF, member id 0xFFFFFFFF.  TM_ENOMEM as
 * tm_set_subscribers.
 *
 * tm_share_state_set / tm_share_state_get: one u32 state word per slot,
 * resident on the device, one array per device entry (`dev`: the position in
 * tm_create_replicas' device list, 0 after tm_create); it grows with its
 * contents kept, and a slot never set holds TM_SHARE_UNDEF (0xFFFFFFFF).  What
 * the word means is the strategy's business (the table below): round_robin's
 * last idx, round_robin_per_group's counter in [0, cnt], sticky's idx.  set is
 * seen by every pick queued after it returns, on every device entry, and by
 * none queued before; get returns the state after every pick queued before it
 * on that entry (a slot beyond the array: TM_SHARE_UNDEF).  Both wait for the
 * entry's batches in flight: control-plane calls.  Both move one copy per run
 * of consecutive slots among those named, so the cost follows n, not the
 * distance between the slots; the array itself holds 4 bytes per slot up to
 * the largest one set or named by a record.  With topic-sharded replicas
 * each device entry advances its OWN state from the messages it is given: the
 * entries' round robins are independent, as the reference's publishing
 * processes are.
 *
 * tm_share_pick_dev: device buffers, asynchronous on `stream`.  d_slot_of ==
 * NULL: the index's own tables and state (the six arguments after it are
 * ignored); else slot_of_len values, n_slots records (16-byte aligned) and
 * n_slots state words, pool_len pool words.  d_key_clientid / d_key_topic: the
 * BEAM's phash2 of the message's sender / topic, one word per topic (NULL: all
 * zero).  cap is clamped to 2^32 - 1.  In numpy:
 *   E = min(doff[n_dests+1], cap);  t, v = topic[:E], value[:E]
 *   s = slot_of[v] where v < slot_of_len, else NONE;  s = NONE where s >= n_slots
 *   pos, cnt, n_local, meta = rec[s];  cnt = 0 where pos + cnt > pool_len
 *                                      (64-bit sum: such a list is never read)
 *   n_local = min(n_local, cnt);  strategy = meta & 0xFF
 *   out_member[q] = 0xFFFFFFFF where s is NONE, cnt == 0 or strategy >= 7; no
 *     state moves for those
 *   cnt == 1: out_member[q] = pool[pos]; no state moves, but under
 *     TM_SHARE_STICKY state[s] = 0
 *   else the entry is active: k = its rank among the active entries of slot s in
 *     ascending q, m = their number, c0 = state[s] before the call; all sums in
 *     64 bits; key_*[t] = 0 for a NULL array or t >= n_topics:
 *       strategy               idx of rank k                            state[s] after
 *       ROUND_ROBIN            c0 == UNDEF: (R(~0, s) % cnt + k) % cnt  idx of rank m - 1
 *                              else (c0 + 1 + k) % cnt
 *       ROUND_ROBIN_PER_GROUP  (min(c0 == UNDEF ? 0 : c0, cnt) + k)     idx of rank m - 1,
 *                                % cnt                                    plus 1
 *       STICKY                 c0 < cnt: c0; else the init_strategy     that idx
 *                              idx of the rank-0 entry, for every rank
 *       RANDOM                 R(t_q, s) % cnt                          unchanged
 *       LOCAL                  n_local == 0: R(t_q, s) % cnt;           unchanged
 *                              n_local == 1: 0; else R(t_q, s) % n_local
 *       HASH_CLIENTID          key_clientid[t_q] % cnt                  unchanged
 *       HASH_TOPIC             key_topic[t_q] % cnt                     unchanged
 *     out_member[q] = pool[pos + idx]
 *   head = [entries with a slot, entries with a pick]
 *   R(a, b): x = seed ^ a * 0x9E3779B1 ^ b * 0x85EBCA77 (u32); x ^= x >> 16;
 *     x *= 0x85EBCA6B; x ^= x >> 13; x *= 0xC2B2AE35; x ^= x >> 16
 * Nothing at or past E is written; the inputs are not modified; no input
 * position >= E and no pool word >= pool_len is read.  The two round-robin rows
 * and the two hash rows are the reference's arithmetic exactly, given the same
 * start state and the same phash2 words (round_robin: Rem = (N + 1) rem Count,
 * Nth = Rem + 1, a fresh process starting at rand:uniform(Count) - 1;
 * per_group: ets:update_counter(.., {2, 1, Count, 1}, {.., 0})); random and
 * local can match it only in distribution.  Two calls on different streams of
 * one device each apply their whole transition of a slot's state atomically --
 * one lane per (call, slot) runs a compare-and-swap loop on the word, no block
 * waits for another -- so the result is that of the two calls in some order.
 * The rank comes from a stable least-significant-digit-first sort of the active
 * entries' (slot, q) pairs, ceil(bits(n_slots - 1) / 9) digit passes of the
 * fan-out's kind over its fixed grid: it does not depend on timing.  The
 * stream's scratch (kept with the fan-out's, tm_stream_release) holds 20 bytes
 * x cap, the fan-out's 8 MiB pass table and 48 KiB (TM_ENOMEM if that cannot be
 * had); size cap from the buffers, as for tm_dispatch_dev.  With the index's
 * own tables one more thing can wait: when the records name more slots than
 * the entry's state array holds, the array grows here -- it is copied, so the
 * call first waits for the entry's batches in flight on every stream (once per
 * growth by half; every other device-API call waits for nothing).  TM_EINVAL before
 * any device work: a null handle, a null required pointer, n_dests == 0 or
 * n_dests > 65536, d_slot_of given with n_slots > 0 but without d_slot_rec or
 * d_state, d_pool NULL while pool_len > 0, d_slot_rec not 16-byte aligned,
 * n_slots > 2^32 - 1.
 *
 * tm_publish_batch: the host product path -- tm_dispatch_batch plus the pick,
 * on the same lane.  flags must hold TM_ROUTE_AGGRE (the reference always runs
 * aggre/1 before route/2): TM_EINVAL without it.  key_clientid / key_topic:
 * host arrays of n words (may be NULL); out_member has cap words, aligned with
 * out_topic / out_values: out_member[q] is the pick of kept entry q with the
 * index's own tables and the state of the device entry the batch ran on; only
 * the first K = out_dest_offsets[n_dests + 1] words are written.  Everything
 * else -- the route outputs, the head and the deliveries, TM_ECAP, lanes,
 * read-your-writes, the retry after a device failure -- is tm_dispatch_batch's
 * to the letter.  The state advances exactly once per successful call: the
 * pick is queued once, after the run that stands (a value scratch that grew, a
 * look-back retry and a delivery scratch that grew all lie before it) and after
 * the route outputs have reached the caller's buffers.  What can still fail
 * behind it is the copy of out_member itself and of the deliveries: the call
 * then returns TM_EDEVICE with the state moved, and the caller reads the words
 * back (tm_share_state_get) rather than resubmitting blindly.  Snapshots: the
 * match, the fan-out, aggre/1 and the dispatch see the index and its tables as
 * of the run; the pick sees the share tables (slots, members, state) as of the
 * moment it is queued, behind that run -- the index lock is not held in
 * between, so a tm_set_share_* or tm_share_state_set that returns meanwhile is
 * seen by the pick though not by the route.  A caller that needs one snapshot
 * keeps such writes out of a batch's call, as the reference's single
 * gen_server does for the tables it mirrors.  Under
 * TM_ECAP from cap (total > cap) no pick is made and no state moves: the
 * caller resubmits.  Under TM_ECAP from dcap alone the route outputs and the
 * picks stand.  TM_EINVAL also for a null out_member with cap > 0.
 *
 * tm_publish_batch32 (ABI minor 19): tm_publish_batch with 32-bit offsets in
 * and out, for a NIF's micro-batches (its C half: c_src/tmatch_nif_share.h).
 * For the same index state, arguments and start state of the slots the return
 * code, every route output, the head, the deliveries, out_member[0 .. K) and
 * the state words afterwards are tm_publish_batch's, out_dest_offsets narrowed
 * to u32 as in tm_dispatch_batch32.  Nothing is written at or past min(total,
 * cap), min(T, dcap), or K in out_member.  Under TM_ECAP from cap no pick is
 * made and no state moves; under TM_ECAP from dcap alone the picks stand; the
 * state moves exactly once per successful call.  TM_EINVAL: whatever
 * tm_dispatch_batch32 refuses, a missing TM_ROUTE_AGGRE, a null out_member
 * with cap > 0.  In place -- one synchronisation, no copy in or out -- under
 * exactly tm_dispatch_batch32's conditions with out_member, and each key array
 * that is given, in this index's tm_host_alloc memory as well: behind the
 * dispatch's workgroup, in the same hold of the index lock and on the same
 * stream, ONE more workgroup picks for the K <= 16384 kept entries on the lane;
 * the ranks come from a stable sort by slot inside its LDS (8-bit digits, as
 * many passes as the largest slot present needs), one lane per (call, slot)
 * applies the transition with the compare-and-swap loop on the device-resident
 * word, so concurrent calls compose as tm_share_pick_dev's do.  The pick then
 * sees the share tables (slots, members, state) of the run's own snapshot:
 * stricter than tm_publish_batch's "as of the moment it is queued", never
 * looser.  That run may have to be run again (a value scratch that grows, a
 * failed batch), so the workgroup gates itself on the device: it picks and
 * moves state only when the fan-out completed, the value scratch held the
 * batch, total <= cap and the lane's fail word is down, and reports which into
 * the lane's status words; the host requires "picked" exactly when the run
 * that stands gives the caller its entries (TM_EDEVICE otherwise).  A local
 * bucket with more deliveries than the dispatch's workgroup expands: the picks
 * are made, the grid kernels finish the deliveries.  A batch with more than
 * 16384 entries: the grid fan-out and dispatch as under tm_dispatch_batch32,
 * then, once the route outputs are out and total <= cap, the grid pick once, as
 * in tm_publish_batch.  Every other batch is widened, run by tm_publish_batch,
 * and narrowed.  TM_DEBUG_PUBLISH_ONE / TM_DEBUG_PUBLISH_GRID count the calls
 * the one-launch kernel picked for / the grid pick or the staged path
 * finished. */
#define TM_SHARE_NONE 0xFFFFFFFFu
#define TM_SHARE_UNDEF 0xFFFFFFFFu
enum { TM_SHARE_RANDOM = 0, TM_SHARE_ROUND_ROBIN = 1, TM_SHARE_ROUND_ROBIN_PER_GROUP = 2, TM_SHARE_STICKY = 3,
       TM_SHARE_LOCAL = 4, TM_SHARE_HASH_CLIENTID = 5, TM_SHARE_HASH_TOPIC = 6 };
int tm_set_share_slots(tm_index *h, uint64_t n, const uint32_t *values, const uint32_t *slots);
int tm_set_share_members(tm_index *h, uint64_t n, const uint32_t *slots, const uint64_t *list_offsets,
                         const uint32_t *members, const uint32_t *n_local, const uint32_t *meta);
int tm_share_state_set(tm_index *h, uint64_t n, const uint32_t *slots, const uint32_t *states);
int tm_share_state_get(tm_index *h, uint32_t dev, uint64_t n, const uint32_t *slots, uint32_t *out);
int tm_share_pick_dev(tm_index *h, uint32_t n_dests, const uint64_t *d_dest_offsets,
                      const uint32_t *d_topic, const uint32_t *d_value, uint64_t cap,
                      const uint32_t *d_key_clientid, const uint32_t *d_key_topic, uint64_t n_topics,
                      uint32_t seed,
                      const uint32_t *d_slot_of, uint64_t slot_of_len,
                      const uint32_t *d_slot_rec, uint64_t n_slots,
                      const uint32_t *d_pool, uint64_t pool_len, uint32_t *d_state,
                      uint64_t *d_out_head, uint32_t *d_out_member, void *stream);
int tm_publish_batch(tm_index *h, uint64_t n, const uint8_t *topic_bytes, const uint64_t *topic_offsets,
                     uint32_t n_dests, uint32_t local_dest, uint32_t flags,
                     uint64_t *out_dest_offsets, uint32_t *out_topic, uint32_t *out_values, uint64_t cap,
                     uint64_t *out_head, uint32_t *out_dtopic, uint32_t *out_dvalue, uint32_t *out_dsub,
                     uint64_t dcap, const uint32_t *key_clientid, const uint32_t *key_topic, uint32_t seed,
                     uint32_t *out_member, uint8_t *out_err);
int tm_publish_batch32(tm_index *h, uint64_t n, const uint8_t *topic_bytes, const uint32_t *topic_offsets,
                       uint32_t n_dests, uint32_t local_dest, uint32_t flags,
                       uint32_t *out_dest_offsets, uint32_t *out_topic, uint32_t *out_values, uint64_t cap,
                       uint64_t *out_head, uint32_t *out_dtopic, uint32_t *out_dvalue, uint32_t *out_dsub,
                       uint64_t dcap, const uint32_t *key_clientid, const uint32_t *key_topic, uint32_t seed,
                       uint32_t *out_member, uint8_t *out_err);

/* Deliveries grouped by subscriber on the device (ABI minor 20).  The calls
 * above end with the local node's deliveries (message, route value,
 * subscriber) in message order; their consumer is one process per subscriber:
 * do_dispatch2/3 sends SubPid ! {deliver, To, Msg} (emqx_broker.erl:745-752),
 * and a connection process first gathers its mailbox's delivers back into one
 * list (emqx_connection.erl:611-612, emqx_channel.erl:1099-1137).  For a
 * micro-batched broker the hand-off is one list per subscriber per batch, the
 * subscriber's deliveries in publish order.
 *
 * tm_group_subs_dev: device buffers, asynchronous on `stream`.  The input is
 * what tm_dispatch_dev wrote: d_head = [M, T] (read on the device, so the call
 * chains behind tm_dispatch_dev with no host synchronisation) and the three
 * delivery arrays, of which cap were there to be written.  cap is clamped to
 * 2^32 - 1.  In numpy:
 *   W = min(head[1], cap);  s = sub[:W]
 *   p = argsort(s, kind="stable")                      -- u32 positions
 *   out_topic, out_value, out_sub = topic[p], value[p], s[p];  out_perm = p  (when given)
 *   gs, cnt = unique(s, return_counts=True);  G = len(gs);  Gw = min(G, gcap)
 *   out_gsub[:Gw] = gs[:Gw];  out_goff[0..Gw] = concatenate([0], cumsum(cnt))[:Gw + 1]
 *   ghead = [G, W]
 * Groups come in ascending subscriber id (unsigned); inside a group the
 * deliveries keep their input order -- the order that preserves MQTT's
 * per-subscriber ordering.  Every u32 is a legal id, 0 and 0xFFFFFFFF included.
 * Nothing at or past W is written in the four per-delivery outputs, nothing at
 * or past Gw in d_out_gsub and nothing past d_out_goff[Gw] (d_out_goff holds
 * gcap + 1 words; entry 0 is written whatever gcap is); the inputs are not
 * modified and no input position >= W is read.  The outputs MUST NOT overlap
 * the inputs.  The grouped per-delivery arrays are complete whatever gcap is;
 * G > gcap: the caller reruns with room for G; ghead is exact either way.
 * A stable least-significant-digit radix sort of (subscriber, position) pairs
 * in 8-bit digits over a fixed grid -- per pass a per-block histogram, a scan
 * and a scatter that ranks stably inside the block -- then the group heads are
 * flagged and scanned and the payload gathered; every step a launch of its own
 * in stream order, no block waiting for another.  A digit on which all W ids
 * agree is skipped on the device (interned ids are dense: ids below 2^16 cost
 * two passes, not four) with the same results; TM_DEBUG_GROUP_PASSES_RUN /
 * _SKIPPED count both.  The stream's scratch (kept with the fan-out's and the
 * dispatch's, tm_stream_release) holds 16 bytes x cap and 1.1 MiB (TM_ENOMEM
 * if that cannot be had, as for tm_dispatch_dev).  It is sized from cap, not
 * from T, which only the device knows when the call is queued: pass the size
 * of the buffers, never 2^32 - 1 for "no bound" -- that asks for about 70 GB a
 * stream.  TM_EINVAL before any device work: a null handle, a null required
 * pointer (d_head, d_out_ghead, d_out_goff; the six arrays when cap > 0;
 * d_out_gsub when gcap > 0), d_head, d_out_ghead or d_out_goff not 8-byte
 * aligned.
 *
 * tm_deliver_batch: the host product path -- tm_dispatch_batch with the same
 * arguments, followed on the same lane and in the same run by the grouping of
 * the local bucket's deliveries.  The route outputs, out_head and every
 * TM_ECAP rule are tm_dispatch_batch's; the three delivery arrays arrive
 * GROUPED (tm_group_subs_dev's out_topic / out_value / out_sub over the first
 * min(T, dcap) deliveries), out_ghead = [G, W], out_gsub takes the first
 * min(G, gcap) subscribers and out_goff (gcap + 1 words) their offsets and
 * the end of the last.  TM_ECAP also when G > gcap: out_ghead[0] sizes the
 * retry.  When the lane's delivery scratch was short the dispatch and the
 * grouping are queued again on the results still in the lane: never a second
 * walk.  flags: 0 or TM_ROUTE_AGGRE.  TM_EINVAL: whatever tm_dispatch_batch
 * refuses, a null out_ghead or out_goff, a null out_gsub with gcap > 0.
 * Lanes, read-your-writes, the device-failure retry and the out_err rules are
 * unchanged. */
int tm_group_subs_dev(tm_index *h, const uint64_t *d_head,
                      const uint32_t *d_topic, const uint32_t *d_value, const uint32_t *d_sub, uint64_t cap,
                      uint64_t *d_out_ghead, uint32_t *d_out_gsub, uint64_t *d_out_goff, uint64_t gcap,
                      uint32_t *d_out_topic, uint32_t *d_out_value, uint32_t *d_out_sub,
                      uint32_t *d_out_perm, void *stream);
int tm_deliver_batch(tm_index *h, uint64_t n, const uint8_t *topic_bytes, const uint64_t *topic_offsets,
                     uint32_t n_dests, uint32_t local_dest, uint32_t flags,
                     uint64_t *out_dest_offsets, uint32_t *out_topic, uint32_t *out_values, uint64_t cap,
                     uint64_t *out_head, uint32_t *out_dtopic, uint32_t *out_dvalue, uint32_t *out_dsub,
                     uint64_t dcap, uint64_t *out_ghead, uint32_t *out_gsub, uint64_t *out_goff, uint64_t gcap,
                     uint8_t *out_err);

/* tm_deliver_batch32 (ABI minor 21): tm_deliver_batch with 32-bit offsets in
 * and out, for the NIF's micro-batches.  For the same index state and
 * arguments the return code and every output are tm_deliver_batch's:
 * out_dest_offsets narrowed to u32 as in tm_dispatch_batch32, out_goff
 * narrowed to u32 (gcap + 1 words; entry 0 is written whatever gcap is);
 * out_head and out_ghead stay u64[2] and must be 8-byte aligned.  Nothing is
 * written at or past min(total, cap) in out_topic / out_values, min(T, dcap)
 * in the three delivery arrays, min(G, gcap) in out_gsub, nor past
 * out_goff[min(G, gcap)].  TM_ECAP: tm_deliver_batch's three rules (total >
 * cap, T > dcap, G > gcap: out_ghead[0] sizes the retry).  TM_EINVAL: whatever
 * tm_dispatch_batch32 refuses, a null out_ghead or out_goff, a null out_gsub
 * with gcap > 0, a misaligned out_ghead.  flags: 0 or TM_ROUTE_AGGRE; there is
 * no pick.
 * In place -- no staging copy, no copy out, one synchronisation -- when
 * tm_dispatch_batch32's conditions hold and out_ghead, out_gsub and out_goff
 * lie in this index's tm_host_alloc memory too; the device never reads a
 * caller's buffer.  The one-workgroup dispatch then leaves its deliveries on
 * the device and ONE more workgroup behind it, on the same stream and under
 * the same hold of the index lock, sorts their subscriber ids inside LDS
 * (stable 8-bit LSD passes over 16-bit positions, a digit all ids agree on
 * skipped as in tm_group_subs_dev) and writes the grouped arrays, the groups
 * and both heads into the caller's buffers.  It takes at most 16384
 * deliveries (TM_DEBUG_GS1_MAX lowers that, TM_DEBUG_DP1_MAX too: the smaller
 * wins): more than that, or more than 16384 route entries, and the grid
 * dispatch and the grid grouping run on the arrays still on the device and
 * the results are copied out -- never a second walk.  Every other batch is
 * widened, run by tm_deliver_batch, and narrowed. */
int tm_deliver_batch32(tm_index *h, uint64_t n, const uint8_t *topic_bytes, const uint32_t *topic_offsets,
                       uint32_t n_dests, uint32_t local_dest, uint32_t flags,
                       uint32_t *out_dest_offsets, uint32_t *out_topic, uint32_t *out_values, uint64_t cap,
                       uint64_t *out_head, uint32_t *out_dtopic, uint32_t *out_dvalue, uint32_t *out_dsub,
                       uint64_t dcap, uint64_t *out_ghead, uint32_t *out_gsub, uint32_t *out_goff, uint64_t gcap,
                       uint8_t *out_err);

/* Shared-subscription picks grouped with the deliveries (ABI minor 22).  One
 * connection process receives both kinds of delivery in one mailbox: {deliver,
 * To, Msg} from do_dispatch2/2 (emqx_broker.erl:726-760) and from the shared
 * dispatch/3 (emqx_shared_sub.erl:146-163).  tm_publish_batch leaves its
 * deliveries in message order and makes the picks; tm_deliver_batch groups by
 * subscriber and makes no pick.  The calls below close the chain: one list per
 * local subscriber, direct and picked deliveries together, in publish order.
 *
 * tm_set_member_subs: the index's share member id -> local subscriber id table,
 * a twin of tm_set_dests (same thread safety, upload discipline and errors).
 * Member ids are tm_set_share_members', subscriber ids tm_set_subscribers'.
 * TM_SHARE_NONE (0xFFFFFFFF): not a connection of this node, and so is a member
 * never set -- such a pick stays a pick in out_member for the host to forward
 * and is never a local delivery.  A local subscriber whose id is 0xFFFFFFFF can
 * therefore not be the target of a merged pick; direct deliveries may still
 * carry that id, as in tm_group_subs_dev.
 *
 * tm_group_picks_dev: device buffers, asynchronous on `stream`.  d_head,
 * d_topic, d_value, d_sub and cap are what tm_dispatch_dev wrote (the
 * deliveries in ascending message order, as it writes them: the merge searches
 * them); n_dests, d_dest_offsets, d_etopic, d_evalue and ecap what tm_aggre_dev
 * wrote; d_member what tm_share_pick_dev wrote.  d_head and the offsets are
 * read on the device, so the call chains behind tm_dispatch_dev and
 * tm_share_pick_dev with no host synchronisation.  d_sub_of == NULL: the
 * index's own tm_set_member_subs table (sub_of_len is then ignored).  cap, ecap
 * and out_cap are clamped to 2^32 - 1.  In numpy:
 *   W = min(head[1], cap);  E = min(doff[n_dests + 1], ecap)
 *   m  = member[:E]
 *   ls = where(m < sub_of_len, sub_of[m], NONE)          # NONE = 0xFFFFFFFF: no pick, or not local
 *   pq = nonzero(ls != NONE)[0];  P = len(pq);  N = W + P
 *   t = concatenate(topic[:W], etopic[pq]);  v = concatenate(value[:W], evalue[pq]);  s = concatenate(sub[:W], ls[pq])
 *   p = lexsort((t, s))            # by subscriber, then by message, then by place in the concatenation: stable
 *   out_topic, out_value, out_sub, out_src = t[p], v[p], s[p], p      -- the first min(N, out_cap); out_src when given
 *   gs, cnt = unique(s, return_counts=True);  G = len(gs);  Gw = min(G, gcap)
 *   out_gsub[:Gw] = gs[:Gw];  out_goff[0..Gw] = concatenate([0], cumsum(cnt))[:Gw + 1];  ghead = [G, N]
 * Inside a subscriber's list the messages ascend; inside one message the direct
 * deliveries come first in their input order, then that message's picks in
 * ascending entry position.  out_src[j] < W names a direct delivery, out_src[j]
 * >= W is W + the pick's rank among the local picks.  (The order of several
 * deliveries of one message to one subscriber has no meaning in MQTT; the rule
 * only has to be fixed.)  With P = 0 every output equals tm_group_subs_dev's
 * for the same deliveries.  Nothing at or past min(N, out_cap) is written in
 * the four per-delivery outputs, nothing at or past Gw in d_out_gsub and
 * nothing past d_out_goff[Gw] (entry 0 is written whatever gcap is); ghead is
 * exact whatever the caps are; the inputs are not modified; no delivery
 * position >= W, no entry position >= E and no d_sub_of word >= sub_of_len is
 * read.  The outputs MUST NOT overlap the inputs.  Steps, each a launch of its
 * own over a fixed grid, no block waiting for another: the local picks are
 * flagged (member, then sub_of), counted per block (ballot, popcount), the
 * counts scanned, and (topic, value, subscriber) compacted in ascending entry
 * position; the P picks are sorted stably by message with tm_group_subs_dev's
 * 8-bit digit passes (a digit all agree on skipped: a batch of at most 256
 * messages costs one pass); picks and deliveries are merged by message through
 * two binary searches on sorted arrays; tm_group_subs_dev's passes then sort
 * the merged deliveries by subscriber.  TM_DEBUG_GROUP_PASSES_RUN / _SKIPPED
 * count both sorts' passes.  The stream's scratch (kept with the fan-out's,
 * tm_stream_release) holds 32 bytes x (cap + ecap), 12 bytes x ecap and 1.1
 * MiB (TM_ENOMEM if that cannot be had).  It is sized from cap + ecap, never
 * from counts only the device knows: pass the sizes of the buffers.  TM_EINVAL
 * before any device work: a null handle, a null required pointer (d_head,
 * d_dest_offsets, d_out_ghead, d_out_goff; the three delivery arrays when cap >
 * 0; d_etopic, d_evalue and d_member when ecap > 0; the three outputs when
 * out_cap > 0; d_out_gsub when gcap > 0), n_dests == 0 or n_dests > 65536,
 * d_head, d_dest_offsets, d_out_ghead or d_out_goff not 8-byte aligned, a given
 * d_sub_of with sub_of_len > 2^32 - 1, min(cap, 2^32 - 1) + min(ecap, 2^32 - 1)
 * > 2^32 - 1 (positions are u32).
 *
 * tm_publish_deliver_batch: the host product path.  It is tm_publish_batch to
 * the letter for the route outputs, out_head = [M, T] (the direct deliveries
 * alone), out_member[0 .. K), the state words, lanes, read-your-writes, the
 * device-failure retry and the required TM_ROUTE_AGGRE.  The three delivery
 * arrays come back merged and grouped: tm_group_picks_dev's outputs over the
 * lane's deliveries and the lane's picks with the index's own
 * tm_set_member_subs table (as of the moment the pick is queued); out_ghead =
 * [G, N], out_gsub and out_goff as in tm_deliver_batch.  The pick and, in the
 * same hold of the index lock and on the same lane, the merge and the grouping
 * are queued once, after the run that stands and after every scratch they need
 * has been had.  The state moves exactly once per successful call and never
 * for a call the caller has to repeat:
 *   total > cap     TM_ECAP, no pick, no state (tm_publish_batch's rule).
 *   T + K > dcap    TM_ECAP, no pick, no state: T and K are known on the host
 *                   before the pick is queued, and K bounds the local picks.
 *                   out_head[1] and out_dest_offsets[n_dests + 1] size the
 *                   retry: dcap >= T + K.  Deliberately stricter than
 *                   tm_publish_batch's dcap rule, under which the picks stand.
 *   under either of these the delivery arrays and the group outputs are not
 *   written and out_ghead = [0, 0].
 *   G > gcap alone  TM_ECAP with the picks made and the state moved once; the
 *                   grouped per-delivery arrays are complete and out_ghead is
 *                   exact: the caller reads the group bounds off the sorted
 *                   out_dsub and does NOT resubmit.
 * TM_EINVAL: whatever tm_publish_batch refuses, a null out_ghead or out_goff,
 * a null out_gsub with gcap > 0. */
int tm_set_member_subs(tm_index *h, uint64_t n, const uint32_t *members, const uint32_t *sub_ids);
int tm_group_picks_dev(tm_index *h, const uint64_t *d_head,
                       const uint32_t *d_topic, const uint32_t *d_value, const uint32_t *d_sub, uint64_t cap,
                       uint32_t n_dests, const uint64_t *d_dest_offsets, const uint32_t *d_etopic,
                       const uint32_t *d_evalue, const uint32_t *d_member, uint64_t ecap,
                       const uint32_t *d_sub_of, uint64_t sub_of_len,
                       uint64_t *d_out_ghead, uint32_t *d_out_gsub, uint64_t *d_out_goff, uint64_t gcap,
                       uint32_t *d_out_topic, uint32_t *d_out_value, uint32_t *d_out_sub, uint32_t *d_out_src,
                       uint64_t out_cap, void *stream);
int tm_publish_deliver_batch(tm_index *h, uint64_t n, const uint8_t *topic_bytes, const uint64_t *topic_offsets,
                             uint32_t n_dests, uint32_t local_dest, uint32_t flags,
                             uint64_t *out_dest_offsets, uint32_t *out_topic, uint32_t *out_values, uint64_t cap,
                             uint64_t *out_head, uint32_t *out_dtopic, uint32_t *out_dvalue, uint32_t *out_dsub,
                             uint64_t dcap, const uint32_t *key_clientid, const uint32_t *key_topic, uint32_t seed,
                             uint32_t *out_member, uint64_t *out_ghead, uint32_t *out_gsub, uint64_t *out_goff,
                             uint64_t gcap, uint8_t *out_err);

/* tm_publish_deliver_batch32 (ABI minor 23): tm_publish_deliver_batch with
 * 32-bit offsets in and out, for the NIF's micro-batches: the last link of the
 * publish chain in place.  For the same index state, arguments and start state
 * of the slots the return code, every route output, out_head = [M, T],
 * out_member[0 .. K), the merged and grouped delivery arrays, out_ghead = [G,
 * N], out_gsub, out_goff and the state words afterwards are
 * tm_publish_deliver_batch's: out_dest_offsets narrowed to u32 as in
 * tm_publish_batch32, out_goff narrowed to u32 (gcap + 1 words; entry 0 is
 * written whatever gcap is); out_head and out_ghead stay u64[2] and must be
 * 8-byte aligned.  Nothing is written at or past min(total, cap) in out_topic /
 * out_values, K in out_member, min(N, dcap) in the three delivery arrays,
 * min(G, gcap) in out_gsub, nor past out_goff[min(G, gcap)].  TM_ECAP:
 * tm_publish_deliver_batch's three rules, to the letter:
 *   total > cap     no pick, no state.
 *   T + K > dcap    no pick, no state; nothing is written to the delivery
 *                   arrays, the group outputs or out_member, out_ghead = [0,
 *                   0]; out_head and the bucket offsets size the retry.
 *   G > gcap alone  the picks stand and the state has moved once; the grouped
 *                   arrays are complete and out_ghead is exact.
 * TM_EINVAL: whatever tm_publish_batch32 refuses, a null out_ghead or
 * out_goff, a null out_gsub with gcap > 0, a misaligned out_ghead.
 * In place -- no staging copy, no copy out, one synchronisation, everything
 * queued in one hold of the index lock on the lane's stream -- when
 * tm_publish_batch32's conditions hold and out_ghead, out_gsub and out_goff lie
 * in this index's tm_host_alloc memory too; the device never reads a caller's
 * buffer.  Behind the walk, the fan-out and the aggre pass the one-workgroup
 * dispatch leaves its deliveries on the device; one wave (the gate) then
 * decides, on the device and once, whether the run stands (tm_publish_batch32's
 * own conditions), T + K <= dcap and one workgroup takes them, and writes
 * out_head; the one-workgroup pick of tm_publish_batch32 picks and moves the
 * state exactly when the gate says so; and ONE more workgroup copies the picks
 * to out_member, flags the local ones against the tm_set_member_subs table,
 * compacts them, sorts them by message, merges them with the deliveries by
 * binary searches and sorts the merged deliveries by subscriber, all inside
 * LDS, and writes the grouped arrays, the groups and out_ghead into the
 * caller's buffers.  The member-subs table is uploaded in the same hold of the
 * lock as the walk is queued in: it is the run's own snapshot, which is
 * stricter than tm_publish_deliver_batch's "as of the moment the pick is
 * queued", never looser.  That workgroup takes at most 8192 merged deliveries
 * (T + K; TM_DEBUG_GP1_MAX lowers that, TM_DEBUG_GS1_MAX and TM_DEBUG_DP1_MAX
 * too: the smallest wins).  More than that, or more than 16384 route entries:
 * no pick has been made, and the grid dispatch (where needed), the grid pick,
 * merge and grouping run once on the arrays still on the device and the
 * results are copied out -- never a second walk.  The one-workgroup ending
 * does everything or moves nothing.  Every other batch is widened, run by
 * tm_publish_deliver_batch, and narrowed. */
int tm_publish_deliver_batch32(tm_index *h, uint64_t n, const uint8_t *topic_bytes, const uint32_t *topic_offsets,
                               uint32_t n_dests, uint32_t local_dest, uint32_t flags,
                               uint32_t *out_dest_offsets, uint32_t *out_topic, uint32_t *out_values, uint64_t cap,
                               uint64_t *out_head, uint32_t *out_dtopic, uint32_t *out_dvalue, uint32_t *out_dsub,
                               uint64_t dcap, const uint32_t *key_clientid, const uint32_t *key_topic, uint32_t seed,
                               uint32_t *out_member, uint64_t *out_ghead, uint32_t *out_gsub, uint32_t *out_goff,
                               uint64_t gcap, uint8_t *out_err);

/* Release the batch scratch kept for `stream` (after its batches finish);
 * a caller that retires a stream calls this.  No reference counterpart. */
int tm_stream_release(tm_index *h, void *stream);

/* match/2: first hit per topic in traversal order.  out_found[i] = 1 and
 * out_value[i] = value if topic i has a match, 0 otherwise (2 = badarg,
 * 3 = more than 65536 levels). */
int tm_first_batch(tm_index *h, uint64_t n, const uint8_t *topic_bytes, const uint64_t *topic_offsets,
                   uint32_t *out_value, uint8_t *out_found);

/* emqx_topic_index:matches_filter/3 (emqx_topic_index.erl:82-84 ->
 * emqx_trie_search.erl:186-189, filter clauses :291-300): for each of n
 * subscription filters, the values of the word-list keys the reference's
 * ordered search returns, in traversal order (the reference's list is the
 * reverse).  Runs on the device over the keys in Erlang term order (rebuilt
 * after key changes; seconds at 10M keys -- a control-plane call).  Host
 * buffers; out_hit_offsets[n+1] always written; TM_ECAP when the values do
 * not fit `cap` (the first `cap` are written).  out_err[i] = 1 if filter i's
 * walk exceeded its step bound (never for a valid filter). */
int tm_matches_filter(tm_index *h, uint64_t n, const uint8_t *filter_bytes, const uint64_t *filter_offsets,
                      uint64_t *out_hit_offsets, uint32_t *out_values, uint64_t cap, uint8_t *out_err);
/* The same with a flags byte per filter (may be NULL: all plain):
 * TM_KEY_ESCAPED marks a filter given as an escaped word list (the key form
 * above) -- matches_filter(Words, Tab, Opts) with binary words that hold a
 * '/' or equal "+" / "#". */
int tm_matches_filter_ex(tm_index *h, uint64_t n, const uint8_t *filter_bytes, const uint64_t *filter_offsets,
                         const uint8_t *filter_flags, uint64_t *out_hit_offsets, uint32_t *out_values, uint64_t cap,
                         uint8_t *out_err);

int tm_stats(tm_index *h, tm_stats_t *out);

/* Filter-sharded merge (device buffers, asynchronous on `stream`; runs on the
 * current HIP device).  `world` shards matched the same n topics;
 * d_shard_hit_offsets is [world][n+1] (each shard's CSR offsets, starting at
 * 0), d_shard_values is [world][stride] (shard r's values at r*stride).  Writes
 * the merged CSR: d_out_hit_offsets[n+1] and, up to `cap`, d_out_values --
 * topic t's values of shard 0, then shard 1, ..., each in that shard's
 * traversal order (the same value set as one index holding all the keys). */
int tm_merge_shards(uint32_t world, uint64_t n, const uint64_t *d_shard_hit_offsets, const uint32_t *d_shard_values,
                    uint64_t stride, uint64_t *d_out_hit_offsets, uint32_t *d_out_values, uint64_t cap,
                    void *stream);

/* Diagnostics.  While enabled, every match batch records HIP events on its
 * stream around the main walk kernel (k_walk_small for a one-launch batch,
 * k_walk_fast for a two-phase one) and around the whole batch;
 * tm_profile_read() resolves them and returns the accumulated device times
 * (milliseconds) and the number of batches since the last reset. */
int tm_profile_enable(tm_index *h, int enable);
int tm_profile_read(tm_index *h, double *walk_ms, double *batch_ms, uint64_t *batches, int reset);

/* Test hooks (no reference counterpart; tests/test_gpu_parity.py):
 *   TM_DEBUG_LB_SPINS       the look-back wait bound (polls of one word) of the
 *   TM_DEBUG_LB_FAIL_BLOCK  next TM_DEBUG_LB_LAUNCHES one-launch batches, and
 *   TM_DEBUG_LB_LAUNCHES    the block that fails as if its wait expired
 *                           (>= 2^32: none)
 *   TM_DEBUG_PHASES         1: batches of <= 65536 topics take the two-phase
 *                           path too (walk, tails, scan, emit); 0 (default):
 *                           one launch where the index allows it
 *   TM_DEBUG_SMALL_KERNEL   the one-launch kernel of small batches: 0 the
 *                           default; 1 k_walk_small with 16
 *                           lanes per topic; 3 with 8 lanes per topic (2 named
 *                           round 5's one-lane-per-topic kernel, removed:
 *                           TM_EINVAL)
 *   TM_DEBUG_COMBINE        concurrent combined launches of small 32-bit
 *                           in-place host batches (tm_match_batch32_ex): 0 =
 *                           every batch its own launch (default 4)
 *   TM_DEBUG_CMB_GATHER     (study) microseconds a new combined launch waits
 *                           for the callers between two batches to queue
 *                           theirs (0 = none, the default)
 *   TM_DEBUG_SMALL_TICKET   1 (default): k_walk_small's blocks take a
 *                           start-order ticket (see "Forward progress"); 0:
 *                           dispatch order
 *   TM_DEBUG_PATCH_ZC       1 (default): patches up to 64 KiB are read by the
 *                           patch kernel from mapped pinned memory; 0: copied
 *                           to the device first
 *   TM_DEBUG_CMB_SPIN       microseconds a caller waiting in the combiner spins
 *                           before it sleeps (0: sleeps at once)
 *   TM_DEBUG_CMB_LAND       retired (round 6: the combined launch's outputs
 *                           landed from HBM by a copy kernel, measured slower
 *                           and removed): 0 only, TM_EINVAL otherwise
 * tm_debug_get: those settings; TM_DEBUG_COMMITS / _COMMIT_WAITS / _COMMIT_FORCED:
 * tm_commit patches, those that waited for a copy to drain, and those
 * published without an idle copy (per device entry; always so with copies = 1); TM_DEBUG_FAILED_BATCHES (one-launch batches whose look-back
 * failed, host API), TM_DEBUG_RETRIED_BATCHES (of those, run again) and the
 * match launches per kernel path: TM_DEBUG_PATH_PHASES (walk, tails, scan,
 * emit), TM_DEBUG_PATH_SMALL (k_walk_small), TM_DEBUG_PATH_LANE (retired:
 * always 0), TM_DEBUG_COMBINED_LAUNCHES / _BATCHES: the combiner's
 * launches and the host batches they carried, and TM_DEBUG_WIDE_NODES /
 * TM_DEBUG_DENSE_WIDE: trie nodes with a child bitmap, and those of them
 * dense enough that the walk probes their child table without it.  (Keys
 * 9-11 named the round-4 one-pass kernel's hooks; 9 and 10 now name these,
 * 11 is retired.)  TM_DEBUG_FANOUT_GRID (get only): the one-wave blocks of a
 * fan-out pass (tm_fanout_dev), each owning an equal chunk of the entries.
 * TM_DEBUG_ROUTE_ONE / TM_DEBUG_ROUTE_GRID (get only): tm_route_batch32 calls
 * whose fan-out the one-launch kernel completed / that the grid kernels or the
 * staged path finished.  TM_DEBUG_ANNEX0 / TM_DEBUG_ANNEX1 (get only): the trie
 * node annexed to that vocab-hint slot as depth << 32 | literal children, or
 * all ones while the slot is unused; TM_DEBUG_HINT_AUDIT (get only): vocab
 * entries whose hint of an annexed node differs from what that node's child
 * slot gives, in the host image (always 0).  TM_DEBUG_SUB_COMPACTIONS (get
 * only): how often tm_set_subscribers rewrote its pool tight.
 * TM_DEBUG_DISPATCH_ONE / TM_DEBUG_DISPATCH_GRID (get only): tm_dispatch_batch32
 * calls the one-launch kernel completed / that the grid kernels or the staged
 * path finished.  TM_DEBUG_DP1_MAX (set / get): the deliveries of the local
 * bucket up to which the one-launch kernel expands them itself, clamped to the
 * compiled bound (32768).  TM_DEBUG_PUBLISH_ONE / TM_DEBUG_PUBLISH_GRID (get
 * only): tm_publish_batch32 calls the one-launch pick kernel picked for / that
 * the grid pick or the staged path finished.  TM_DEBUG_GROUP_TILE (get only):
 * the keys a block of tm_group_subs_dev ranks per pass at a time, and
 * TM_DEBUG_GROUP_GRID (get only) the blocks of its fixed grid;
 * TM_DEBUG_GROUP_PASSES_RUN / TM_DEBUG_GROUP_PASSES_SKIPPED (get only): the
 * digit passes the grouping calls that have finished ran / skipped, summed
 * over the streams whose scratch is live (four per call together), and those
 * of tm_deliver_batch32's one-workgroup grouping.  TM_DEBUG_DELIVER_ONE /
 * TM_DEBUG_DELIVER_GRID (get only): tm_deliver_batch32 calls the one-workgroup
 * grouping completed / that the grid kernels or the staged path finished.
 * TM_DEBUG_GS1_MAX (set / get): the deliveries up to which that workgroup
 * groups them itself, clamped to the compiled bound (16384).
 * TM_DEBUG_GP1_MAX (set / get): the merged deliveries (T + K) up to which
 * tm_publish_deliver_batch32's one workgroup merges and groups them itself,
 * clamped to the compiled bound (8192).  TM_DEBUG_PUBLISH_DELIVER_ONE /
 * TM_DEBUG_PUBLISH_DELIVER_GRID (get only): tm_publish_deliver_batch32 calls
 * the one-workgroup ending finished (merged and grouped, or TM_ECAP with
 * nothing moved) / that the grid kernels or the staged path finished.  The
 * one workgroup's digit passes are counted in TM_DEBUG_GROUP_PASSES_RUN /
 * _SKIPPED: four per sort, the picks' by message and the merged deliveries' by
 * subscriber. */
enum { TM_DEBUG_LB_SPINS = 1, TM_DEBUG_LB_FAIL_BLOCK = 2, TM_DEBUG_LB_LAUNCHES = 3, TM_DEBUG_PHASES = 4,
       TM_DEBUG_FAILED_BATCHES = 5, TM_DEBUG_RETRIED_BATCHES = 6, TM_DEBUG_PATH_PHASES = 7,
       TM_DEBUG_PATH_SMALL = 8, TM_DEBUG_PATH_LANE = 9, TM_DEBUG_SMALL_KERNEL = 10,
       TM_DEBUG_COMBINE = 12, TM_DEBUG_COMBINED_LAUNCHES = 13, TM_DEBUG_COMBINED_BATCHES = 14,
       TM_DEBUG_WIDE_NODES = 15, TM_DEBUG_DENSE_WIDE = 16, TM_DEBUG_CMB_GATHER = 17, TM_DEBUG_CMB_LAND = 18,
       TM_DEBUG_COMMITS = 19, TM_DEBUG_COMMIT_WAITS = 20, TM_DEBUG_COMMIT_FORCED = 21, TM_DEBUG_SMALL_TICKET = 22,
       TM_DEBUG_CMB_SPIN = 23, TM_DEBUG_PATCH_ZC = 24, TM_DEBUG_FANOUT_GRID = 25,
       TM_DEBUG_ROUTE_ONE = 26, TM_DEBUG_ROUTE_GRID = 27, TM_DEBUG_ANNEX0 = 28, TM_DEBUG_ANNEX1 = 29,
       TM_DEBUG_HINT_AUDIT = 30, TM_DEBUG_SUB_COMPACTIONS = 31, TM_DEBUG_DISPATCH_ONE = 32,
       TM_DEBUG_DISPATCH_GRID = 33, TM_DEBUG_DP1_MAX = 34, TM_DEBUG_PUBLISH_ONE = 35, TM_DEBUG_PUBLISH_GRID = 36,
       TM_DEBUG_GROUP_TILE = 37, TM_DEBUG_GROUP_PASSES_RUN = 38, TM_DEBUG_GROUP_PASSES_SKIPPED = 39,
       TM_DEBUG_GROUP_GRID = 40, TM_DEBUG_DELIVER_ONE = 41, TM_DEBUG_DELIVER_GRID = 42, TM_DEBUG_GS1_MAX = 43,
       TM_DEBUG_GP1_MAX = 44, TM_DEBUG_PUBLISH_DELIVER_ONE = 45, TM_DEBUG_PUBLISH_DELIVER_GRID = 46 };
int tm_debug_set(tm_index *h, uint32_t key, uint64_t value);
int tm_debug_get(tm_index *h, uint32_t key, uint64_t *value);

/* Last error text of the calling thread (h is ignored; kept for the ABI). */
const char *tm_last_error(tm_index *h);

/* The retained-message store (ABI minor 24): one subscription filter against
 * the stored topic names, emqx_retainer:on_session_subscribed ->
 * emqx_retainer_mnesia:match_messages/3.  A handle of its own, independent of
 * tm_index: a host dictionary interns level words to ids, the rows are columns
 * of ids on the device (the first RT_COLS = 8 levels, deeper ones in an
 * overflow run), rows [0, base) sorted by id sequence and rows
 * [base, base + tail) recent inserts; past tail_max tail rows the store
 * compacts (dead rows dropped, tail merged, dictionary ids with no live row
 * freed).  A stored topic T matches a filter F as emqx_topic:match/2 says
 * (emqx_topic.erl:80-116): levels split on '/', the empty level an ordinary
 * word; a filter level is a wildcard only when it is exactly '+' or '#'; a
 * first level '+' or '#' never matches a topic whose first byte is '$'; a
 * final '#' matches whatever is left, nothing included; without it the level
 * counts are equal.  Calls on one store serialise on its mutex; stores are
 * independent of each other.  A match after a write on the same store sees the
 * write.  The error text of these calls is tm_retained_last_error's, per
 * calling thread. */
typedef struct tm_retained tm_retained;
typedef struct {
    uint32_t initial_rows;   /* rows allocated at first (0 = 1024); the arrays double */
    uint32_t tail_max;       /* tail rows that trigger a compaction (0 = 4096)       */
} tm_retained_opts;
typedef struct {
    uint64_t live_rows, base_rows, tail_rows, dead_rows;
    uint64_t words;             /* dictionary entries                                   */
    uint64_t compactions, growths;
    uint64_t match_launches;    /* tm_retained_match calls that scanned on the device   */
    uint64_t no_launch_filters; /* filters answered on the host alone                   */
    uint64_t device_bytes;
    uint64_t rt_cols, rt_tile;  /* the compiled RT_COLS and RT_TILE                     */
} tm_retained_stats_t;

/* An empty store on a device (-1: the current one).  opts may be NULL.  (The
 * reference's create/1, emqx_retainer_mnesia.erl:143-166, makes the tables.) */
int tm_retained_create(int device, const tm_retained_opts *opts, tm_retained **out);
/* close/1 (emqx_retainer_mnesia.erl:205) keeps the tables; this frees the store
 * and its device memory.  TM_EINVAL for a null handle (as tm_destroy). */
int tm_retained_destroy(tm_retained *r);

/* store_retained (emqx_retainer_mnesia.erl:207-224, 358-384): insert or replace
 * n topics in order, topic i = topic_bytes[topic_offsets[i] .. topic_offsets[i+1]).
 * values[i] is the caller's (any u32), expiry_ms[i] = 0 never expires
 * (expiry_ms may be NULL: all 0).  out_code[i] (may be NULL): 0 replaced, 1 new,
 * 2 invalid topic (empty, a level exactly '+' or '#', more than 65536 levels),
 * which stores nothing.  One staged batch, one kernel (k_ret_apply). */
int tm_retained_put(tm_retained *r, uint64_t n, const uint8_t *topic_bytes, const uint64_t *topic_offsets,
                    const uint32_t *values, const uint64_t *expiry_ms, uint8_t *out_code);

/* delete_message for exact topics (emqx_retainer_mnesia.erl:271-275, 477-494):
 * out_found[i] (may be NULL) = 1 if the topic was stored.  A wildcard delete is
 * a match with now_ms = 0 and a delete of each hit (:277-282), the caller's. */
int tm_retained_delete(tm_retained *r, uint64_t n, const uint8_t *topic_bytes, const uint64_t *topic_offsets,
                       uint8_t *out_found);

/* read_message (emqx_retainer_mnesia.erl:285-286, 502-514): exact topics, host
 * side only.  out_found[i] = 1 and out_value[i] set iff the topic is stored and
 * expiry == 0 || expiry >= now_ms (the read path's >=, :510; the match path
 * below uses >). */
int tm_retained_get(tm_retained *r, uint64_t n, const uint8_t *topic_bytes, const uint64_t *topic_offsets,
                    uint64_t now_ms, uint32_t *out_value, uint8_t *out_found);

/* match_messages for n filters (emqx_retainer_mnesia.erl:288-304, 409-475;
 * emqx_topic.erl:80-116).  A row is visible iff expiry == 0 || expiry > now_ms
 * (:464-466, :518), so now_ms = 0 shows every row (:277).  The result is CSR:
 * the values of filter i's rows are out_values[out_hit_offsets[i] ..
 * out_hit_offsets[i+1]), in no particular order and without duplicates.
 * out_hit_offsets[n+1] always holds the true counts; TM_ECAP if
 * out_hit_offsets[n] > cap (out_values is then unspecified, and nothing is
 * written at or past cap); out_values may be NULL with cap 0 to size a
 * buffer.  out_err[i] (may be NULL) = 2: not a valid filter ('#' not last),
 * its list is empty; else 0. */
int tm_retained_match(tm_retained *r, uint64_t n, const uint8_t *filter_bytes, const uint64_t *filter_offsets,
                      uint64_t now_ms, uint64_t *out_hit_offsets, uint32_t *out_values, uint64_t cap,
                      uint8_t *out_err);

/* clear_expired with msg_expiry_interval_override disabled
 * (emqx_retainer_mnesia.erl:226-269, :231-234): deletes rows with
 * expiry != 0 && expiry < deadline_ms, at most `limit` of them (0 = all) and,
 * where out_values is not NULL, at most cap; their values go to out_values,
 * their number to *out_n.  *out_complete is the reference's Complete: 1 iff the
 * scan reached the table's end before `limit` rows were taken (:266-267: with
 * exactly `limit` expired rows it is 0, and the next call answers 0 rows,
 * complete).  Host side. */
int tm_retained_expire(tm_retained *r, uint64_t deadline_ms, uint64_t limit, uint32_t *out_values,
                       uint64_t cap, uint64_t *out_n, int *out_complete);

/* Compact now: what passing tail_max does (no reference counterpart: mnesia
 * keeps its own tables).  Under a pin (tm_retained_pin) it is deferred. */
int tm_retained_compact(tm_retained *r);

/* table_size (emqx_retainer_mnesia.erl:541-542) is live_rows; the rest is the
 * store's own bookkeeping. */
int tm_retained_stats(tm_retained *r, tm_retained_stats_t *out);

/* Match cursors (ABI minor 25): match_messages/3 as the reference uses it.
 * match_messages(State, Topic, undefined) opens a stream, every later call
 * consumes batch_read_number rows of it (emqx_retainer_mnesia.erl:288-304), and
 * the dispatcher loops over the cursor and ends with delete_cursor
 * (emqx_retainer_dispatcher.erl:248-301).  tm_retained_match is the
 * all_remaining form; tm_retained_match_page returns one bounded page per
 * filter, each filter at its own position.
 *
 * Scan order: a filter's rows are visited first in the base range of its
 * literal prefix by ascending row index, then in the tail by ascending row
 * index, and its values come out in that order (tm_retained_match promises no
 * order).  A cursor is opaque: TM_RET_CURSOR_BEGIN opens, TM_RET_CURSOR_DONE is
 * the end; any other value names the store's epoch (compactions + 1, 24 bits)
 * and the next row to visit (40 bits).  A cursor belongs to the store, not to
 * the filter: handed to another filter it starts at that filter's first row at
 * or after it (below its base range: the range's start; past it: the tail). */
#define TM_RET_CURSOR_BEGIN 0ull
#define TM_RET_CURSOR_DONE  0xFFFFFFFFFFFFFFFFull
#define TM_RET_ESTALE 3      /* out_err[i]: the cursor is of another epoch */

/* One page for each of n filters (emqx_retainer_mnesia.erl:288-304;
 * emqx_utils_stream:consume/2 as :298-304 uses it).  The filter rules, the
 * visibility rule (expiry == 0 || expiry > now_ms), out_err[i] == 2 and the
 * TM_ECAP behaviour are tm_retained_match's: out_hit_offsets[n+1] always holds
 * the true counts, and nothing is written at or past cap.  A filter takes at
 * most `limit` (>= 1) values, so out_hit_offsets[n] <= n * limit and a caller
 * that passes cap = n * limit never sees TM_ECAP: one call, one buffer.
 * cursor_in[i] (NULL: all BEGIN) says where filter i goes on; only rows at or
 * after it are scanned, at most scan_rows of them in this call (0: no bound),
 * base range then tail.  out_cursor[i] is what to pass next:
 *   - `limit` values were found: the row after the limit-th hit, even when that
 *     is the end of the rows.  The next call then returns nothing and DONE, as
 *     the reference returns {ok, [], undefined} after exactly BatchNum rows
 *     were left;
 *   - fewer, and the scan reached the end of the tail: DONE;
 *   - fewer, because scan_rows rows were examined first: the row where the
 *     window stopped.  A short (even empty) page with a live cursor is legal;
 *     the caller calls again.
 * DONE coming in, a literal the dictionary lacks, no rows at or after the
 * cursor and an invalid filter all give an empty list and DONE.
 *
 * Staleness.  Row indices do not move under put, delete, expire or growth; they
 * move only at a compaction, which bumps the epoch.  A cursor of another epoch
 * gets out_err[i] = TM_RET_ESTALE, an empty list and out_cursor[i] = BEGIN: the
 * caller decides whether to start again.  tm_retained_pin keeps the store from
 * compacting while cursors are open.
 *
 * Concurrent writes.  A row written while a cursor is open is seen if it lands
 * at or after the cursor (a new topic goes to the end of the tail; a replaced or
 * re-put topic keeps its row) and not otherwise; a row deleted or expired before
 * the cursor reaches it is not returned.  The reference's ets stream is no
 * stronger.  now_ms is the caller's on every call: pass the one of the first
 * call to keep the reference's Now, captured when the stream is built. */
int tm_retained_match_page(tm_retained *r, uint64_t n, const uint8_t *filter_bytes, const uint64_t *filter_offsets,
                           uint64_t now_ms, const uint64_t *cursor_in, uint32_t limit, uint64_t scan_rows,
                           uint64_t *out_hit_offsets, uint32_t *out_values, uint64_t cap, uint64_t *out_cursor,
                           uint8_t *out_err);

/* Holders of open cursors (emqx_retainer_dispatcher.erl:248-301 holds one from
 * the first read to delete_cursor).  While the count is above 0 the store does
 * not compact: a batch of writes flushes and lets the tail pass tail_max, and
 * tm_retained_compact returns TM_OK with the compaction due.  The
 * tm_retained_unpin that brings the count to 0 compacts if one is due or the
 * tail is past tail_max.  An unpin at count 0 is TM_EINVAL.  With no pin held
 * every other call behaves as it did before ABI minor 25. */
int tm_retained_pin(tm_retained *r);
int tm_retained_unpin(tm_retained *r);

/* Last error text of the calling thread from a tm_retained_* call. */
const char *tm_retained_last_error(tm_retained *r);

/* ABI version: (major << 16) | minor. */
uint32_t tm_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* TMATCH_H */
